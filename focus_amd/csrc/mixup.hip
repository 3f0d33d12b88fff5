// mixup.hip -- Mixup / CutMix of a batch of clips in place, the dense mixed target, and the soft-target cross entropy
// (datasets/mixup.py:40-192 and losses.py:15-36 of the reference).
//
// Pair-wise and in place: sample i is mixed with sample B-1-i, so the thread that owns an element position of the pair
// loads both values, computes both results and stores both.  No flipped copy exists, and no element is read after its
// partner was overwritten: a pair's position is touched by exactly one thread, once.  The clips make 2 passes over memory
// (1 read + 1 write) where the ATen chain flip / mul_ / mul_ / add_ makes 9.
//
// Rounding contract: ATen rounds after each of its three operations, so rnd() below rounds to the tensor's type after each
// of ours, and contraction is switched off for the whole file: an fma would skip the rounding of the product.
#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;     // memory-bound: cap the grid and stride the rest
constexpr int TRIPS = 4;             // grid sized for about this many trips of the loop per thread below the cap

template <typename T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// r(r(a lam) + r(b oml)): three separately rounded operations
template <typename T> __device__ __forceinline__ float mix(float a, float b, float lam, float oml) {
    const float pa = rnd<T>(a * lam);
    const float pb = rnd<T>(b * oml);
    return rnd<T>(pa + pb);
}

// VEC consecutive elements as floats: one 16-byte access (4 fp32 or 8 bf16), or one element
template <typename T, int VEC> __device__ __forceinline__ void ldv(const T* p, float (&f)[VEC]) {
    if constexpr (VEC == 1) {
        f[0] = ld<T>(p);
    } else if constexpr (VEC == 4) {
        const f4 v = ld4<float>(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else {
        ld8<bf16_t>(p, f);
    }
}
template <typename T, int VEC> __device__ __forceinline__ void stv(T* p, const float (&f)[VEC]) {
    if constexpr (VEC == 1) {
        st<T>(p, f[0]);
    } else if constexpr (VEC == 4) {
        st4<float>(p, {f[0], f[1], f[2], f[3]});
    } else {
        st8<bf16_t>(p, f);
    }
}

// work item w = (pair i, vector v of the sample): i = w / nvec < ceil(B/2), partner j = B-1-i >= i
template <typename T, int VEC>
__global__ __launch_bounds__(THREADS) void mixup_blend_kernel(T* __restrict__ x, int64_t B, int64_t n, int64_t nvec,
                                                              int64_t work, float lam, float oml) {
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t w = (int64_t)blockIdx.x * THREADS + threadIdx.x; w < work; w += stride) {
        const int64_t i = w / nvec, v = w - i * nvec, j = B - 1 - i;
        T* pi = x + i * n + v * VEC;
        float a[VEC], oi[VEC];
        ldv<T, VEC>(pi, a);
        if (i == j) {                                            // middle sample of an odd batch: mixed with itself
#pragma unroll
            for (int k = 0; k < VEC; ++k) oi[k] = mix<T>(a[k], a[k], lam, oml);
            stv<T, VEC>(pi, oi);
        } else {
            T* pj = x + j * n + v * VEC;
            float b[VEC], oj[VEC];
            ldv<T, VEC>(pj, b);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                oi[k] = mix<T>(a[k], b[k], lam, oml);
                oj[k] = mix<T>(b[k], a[k], lam, oml);
            }
            stv<T, VEC>(pi, oi);
            stv<T, VEC>(pj, oj);
        }
    }
}

// Rectangle swap.  Work item w = (pair i < B/2, plane m, row y of the rectangle, chunk c of the row); a chunk is the VEC
// columns [c VEC, c VEC + VEC) of the frame's row (16 bytes, aligned, because VEC > 1 is only used when W % VEC == 0 and x
// is 16-byte aligned).  A chunk inside [xl, xh) is swapped with one 16-byte access per sample; a chunk the rectangle's
// edge cuts is swapped element by element, so nothing outside the rectangle is read or written.
template <typename T, int VEC>
__global__ __launch_bounds__(THREADS) void cutmix_paste_kernel(T* __restrict__ x, int64_t B, int64_t M, int H, int W, int yl,
                                                               int rh, int xl, int xh, int c0, int nchunk, int64_t work) {
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    const int64_t plane = (int64_t)H * W;
    for (int64_t w = (int64_t)blockIdx.x * THREADS + threadIdx.x; w < work; w += stride) {
        const int64_t row = w / nchunk;
        const int c = (int)(w - row * nchunk) + c0;
        const int64_t pm = row / rh;
        const int y = (int)(row - pm * rh) + yl;
        const int64_t i = pm / M, m = pm - i * M, j = B - 1 - i;
        T* pi = x + (i * M + m) * plane + (int64_t)y * W;
        T* pj = x + (j * M + m) * plane + (int64_t)y * W;
        const int lo = c * VEC, hi = lo + VEC;
        if (VEC > 1 && lo >= xl && hi <= xh) {
            float a[VEC], b[VEC];
            ldv<T, VEC>(pi + lo, a);
            ldv<T, VEC>(pj + lo, b);
            stv<T, VEC>(pi + lo, b);
            stv<T, VEC>(pj + lo, a);
        } else {
            for (int xx = max(lo, xl); xx < min(hi, xh); ++xx) {
                const T a = pi[xx], b = pj[xx];
                pi[xx] = b;
                pj[xx] = a;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void mixup_target_kernel(const int64_t* __restrict__ labels, float* __restrict__ target,
                                                               int B, int V, float on, float off, float lam, float oml) {
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (int64_t)B * V) return;
    const int b = (int)(idx / V);
    const int64_t c = idx - (int64_t)b * V;
    const float t1 = labels[b] == c ? on : off;                 // a label outside [0,V) equals no column
    const float t2 = labels[B - 1 - b] == c ? on : off;
    target[idx] = mix<float>(t1, t2, lam, oml);
}

// ---- soft-target cross entropy: one block (256 threads) per row, the sibling of xent_ls_kernel (misc.hip) ----------------
// loss = lse sum(y) - sum(y x), evaluated as log(s) sum(y) - sum(y (x - m)) with m = max x, s = sum exp(x - m): the same
// value, without the cancellation of two terms of the size of the logits.
__global__ __launch_bounds__(THREADS) void xent_soft_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                            float* __restrict__ loss_rows, float* __restrict__ dlogits, int R,
                                                            int V) {
    __shared__ float red[16];
    const int r = blockIdx.x;
    const float* x = logits + (int64_t)r * V;
    const float* y = target + (int64_t)r * V;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += THREADS) m = fmaxf(m, x[i]);
    m = block_max(m, red);
    float s = 0.f, sy = 0.f, syx = 0.f;
    for (int i = threadIdx.x; i < V; i += THREADS) {
        const float d = x[i] - m;
        s += expf(d);
        sy += y[i];
        syx += y[i] * d;
    }
    s = block_sum(s, red);
    sy = block_sum(sy, red);
    syx = block_sum(syx, red);
    if (threadIdx.x == 0) loss_rows[r] = logf(s) * sy - syx;
    const float inv_s = 1.f / s, inv_r = 1.f / (float)R;
    for (int i = threadIdx.x; i < V; i += THREADS)
        dlogits[(int64_t)r * V + i] = (expf(x[i] - m) * inv_s * sy - y[i]) * inv_r;
}

inline unsigned grid_for(int64_t work) {
    const int64_t b = cdiv64(work, (int64_t)THREADS * TRIPS);
    return (unsigned)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

}  // namespace

extern "C" int focus_mixup_blend(void* x, int64_t B, int64_t n_per_sample, float lam, float one_minus_lam, int dtype,
                                 void* stream) {
    if (!x) return FOCUS_ERR_NULL;
    if (B < 1 || n_per_sample < 1 || B > INT64_MAX / 4 / n_per_sample) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    const size_t es = focus_esize(dtype);
    if (!focus_aligned(x, es)) return FOCUS_ERR_ALIGN;
    const int vec = (int)(16 / es);
    const bool wide = focus_aligned(x, 16) && n_per_sample % vec == 0;
    const int64_t nvec = wide ? n_per_sample / vec : n_per_sample;
    const int64_t work = ((B + 1) / 2) * nvec;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(grid_for(work));
    if (dtype == FOCUS_BF16) {
        if (wide) mixup_blend_kernel<bf16_t, 8><<<grid, THREADS, 0, s>>>((bf16_t*)x, B, n_per_sample, nvec, work, lam, one_minus_lam);
        else mixup_blend_kernel<bf16_t, 1><<<grid, THREADS, 0, s>>>((bf16_t*)x, B, n_per_sample, nvec, work, lam, one_minus_lam);
    } else {
        if (wide) mixup_blend_kernel<float, 4><<<grid, THREADS, 0, s>>>((float*)x, B, n_per_sample, nvec, work, lam, one_minus_lam);
        else mixup_blend_kernel<float, 1><<<grid, THREADS, 0, s>>>((float*)x, B, n_per_sample, nvec, work, lam, one_minus_lam);
    }
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_cutmix_paste(void* x, int64_t B, int64_t M, int H, int W, int yl, int yh, int xl, int xh, int dtype,
                                  void* stream) {
    if (!x) return FOCUS_ERR_NULL;
    if (B < 1 || M < 1 || H < 1 || W < 1) return FOCUS_ERR_SHAPE;
    if (yl < 0 || yh > H || yl > yh || xl < 0 || xh > W || xl > xh) return FOCUS_ERR_SHAPE;
    if (M > INT64_MAX / 4 / ((int64_t)H * W) || B > INT64_MAX / 4 / ((int64_t)H * W * M)) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    const size_t es = focus_esize(dtype);
    if (!focus_aligned(x, es)) return FOCUS_ERR_ALIGN;
    if (yl == yh || xl == xh || B < 2) return FOCUS_OK;
    const int vec = (int)(16 / es);
    const bool wide = focus_aligned(x, 16) && W % vec == 0;
    const int cv = wide ? vec : 1;
    const int c0 = xl / cv, nchunk = (xh - 1) / cv - c0 + 1, rh = yh - yl;
    const int64_t work = (B / 2) * M * rh * nchunk;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(grid_for(work));
    if (dtype == FOCUS_BF16) {
        if (wide) cutmix_paste_kernel<bf16_t, 8><<<grid, THREADS, 0, s>>>((bf16_t*)x, B, M, H, W, yl, rh, xl, xh, c0, nchunk, work);
        else cutmix_paste_kernel<bf16_t, 1><<<grid, THREADS, 0, s>>>((bf16_t*)x, B, M, H, W, yl, rh, xl, xh, c0, nchunk, work);
    } else {
        if (wide) cutmix_paste_kernel<float, 4><<<grid, THREADS, 0, s>>>((float*)x, B, M, H, W, yl, rh, xl, xh, c0, nchunk, work);
        else cutmix_paste_kernel<float, 1><<<grid, THREADS, 0, s>>>((float*)x, B, M, H, W, yl, rh, xl, xh, c0, nchunk, work);
    }
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_mixup_target(const int64_t* labels, float* target, int B, int V, float on, float off, float lam,
                                  float one_minus_lam, void* stream) {
    if (!labels || !target) return FOCUS_ERR_NULL;
    if (B < 1 || V < 1) return FOCUS_ERR_SHAPE;
    const int64_t blocks = cdiv64((int64_t)B * V, THREADS);
    if (blocks > 0x7fffffff) return FOCUS_ERR_SHAPE;
    mixup_target_kernel<<<dim3((unsigned)blocks), THREADS, 0, (hipStream_t)stream>>>(labels, target, B, V, on, off, lam,
                                                                                    one_minus_lam);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_xent_soft(const float* logits, const float* target, float* loss_rows, float* dlogits, int R, int V,
                               void* stream) {
    if (!logits || !target || !loss_rows || !dlogits) return FOCUS_ERR_NULL;
    if (R < 1 || V < 1) return FOCUS_ERR_SHAPE;
    xent_soft_kernel<<<dim3((unsigned)R), THREADS, 0, (hipStream_t)stream>>>(logits, target, loss_rows, dlogits, R, V);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
