// decode_attn.hip -- one generation step of the STEVE decoder (steve.py:359-381, greedy autoregressive decoding).
//
// focus_decode_attn: attention of ONE new query row per sequence over a key/value cache [B, Lmax, heads*d].  The step is a
// read of len * d keys and values per (sequence, head) against d multiply-adds each: bandwidth, no matrix pipe.  One
// 256-thread workgroup owns a (sequence, head).  G = 1, 2, 4 or 8 neighbouring lanes share a key, lane c of them holding
// channels 8c .. 8c+7 (one 16-byte load of bf16, two of fp32, straight to registers); the 256 / G key slots of the
// workgroup stride over the keys, four keys per slot in flight.  Every slot keeps a running maximum, sum and 8 output
// channels in fp32 (online softmax); the slots are combined once at the end, by shuffles inside a wave and through LDS
// across the four waves.  A key past `len` is neither loaded nor counted: its score is -inf and its values are zeros, so
// whatever the unwritten tail of a cache holds (NaN included) never reaches the result.
// With k_new / v_new the row len-1 of both caches is written from them bit for bit by the lanes that own that key, which
// use the registers they just loaded instead of reading the row back.
//
// focus_greedy_next: the end of a step -- arg-max of a row of logits (lowest index on ties, a NaN counts as the largest
// value, as torch.argmax has it), the token written as int64, and the next input row dict[token] + position row rounded to
// the compute type: argmax + Embedding + cat + position add + cast of the reference loop in one launch.
#include "focus_common.h"

namespace {

constexpr int NT = 256, NW = NT / 64, U = 4;

// 8 consecutive elements as raw bits (what a bit copy moves)
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> { uint4 a; };
template <> struct Raw8<float> { uint4 a, b; };

__device__ __forceinline__ Raw8<bf16_t> ldraw(const bf16_t* p) { return {*reinterpret_cast<const uint4*>(p)}; }
__device__ __forceinline__ Raw8<float> ldraw(const float* p) {
    return {*reinterpret_cast<const uint4*>(p), *reinterpret_cast<const uint4*>(p + 4)};
}
__device__ __forceinline__ void straw(bf16_t* p, const Raw8<bf16_t>& r) { *reinterpret_cast<uint4*>(p) = r.a; }
__device__ __forceinline__ void straw(float* p, const Raw8<float>& r) {
    *reinterpret_cast<uint4*>(p) = r.a;
    *reinterpret_cast<uint4*>(p + 4) = r.b;
}
__device__ __forceinline__ void unpack(const Raw8<bf16_t>& r, float (&f)[8]) {
    f[0] = __uint_as_float(r.a.x << 16); f[1] = __uint_as_float(r.a.x & 0xffff0000u);
    f[2] = __uint_as_float(r.a.y << 16); f[3] = __uint_as_float(r.a.y & 0xffff0000u);
    f[4] = __uint_as_float(r.a.z << 16); f[5] = __uint_as_float(r.a.z & 0xffff0000u);
    f[6] = __uint_as_float(r.a.w << 16); f[7] = __uint_as_float(r.a.w & 0xffff0000u);
}
__device__ __forceinline__ void unpack(const Raw8<float>& r, float (&f)[8]) {
    f[0] = __uint_as_float(r.a.x); f[1] = __uint_as_float(r.a.y); f[2] = __uint_as_float(r.a.z); f[3] = __uint_as_float(r.a.w);
    f[4] = __uint_as_float(r.b.x); f[5] = __uint_as_float(r.b.y); f[6] = __uint_as_float(r.b.z); f[7] = __uint_as_float(r.b.w);
}
template <typename T> __device__ __forceinline__ Raw8<T> zero_raw();
template <> __device__ __forceinline__ Raw8<bf16_t> zero_raw<bf16_t>() { return {make_uint4(0, 0, 0, 0)}; }
template <> __device__ __forceinline__ Raw8<float> zero_raw<float>() { return {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}; }

template <typename T, int LG>
__global__ __launch_bounds__(NT) void decode_attn_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k_new,
                                                         const T* __restrict__ v_new, int64_t ldn, T* __restrict__ kc,
                                                         T* __restrict__ vc, int64_t ldc, int64_t bsc, T* __restrict__ out,
                                                         int64_t ldo, int heads, int d, int len, float scale) {
    constexpr int G = 1 << LG, S = NT / G;               // lanes per key, key slots of the workgroup
    __shared__ float red_m[NW];
    __shared__ float red[NW][G][9];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = tid & (G - 1), slot = tid >> LG;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const bool live = c * 8 < d;                         // d = 48: lanes 6, 7 of every 8 hold no channels
    const int64_t col = (int64_t)h * d + c * 8;
    float qf[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[i] = 0.f;
    if (live) {
        unpack(ldraw(q + (int64_t)b * ldq + col), qf);
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[i] *= scale;
    }
    T* kb = kc + (int64_t)b * bsc + col;
    T* vb = vc + (int64_t)b * bsc + col;
    const int last = k_new ? len - 1 : -1;               // the key that arrives with this call
    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = 0.f;

    for (int base = 0; base < len; base += U * S) {      // the same trip count for every lane: the shuffles below see whole groups
        Raw8<T> kr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = base + u * S + slot;
            kr[u] = zero_raw<T>();
            vr[u] = zero_raw<T>();
            if (live && j < len) {
                if (j == last) {
                    kr[u] = ldraw(k_new + (int64_t)b * ldn + col);
                    vr[u] = ldraw(v_new + (int64_t)b * ldn + col);
                    straw(kb + (int64_t)j * ldc, kr[u]);
                    straw(vb + (int64_t)j * ldc, vr[u]);
                } else {
                    kr[u] = ldraw(kb + (int64_t)j * ldc);
                    vr[u] = ldraw(vb + (int64_t)j * ldc);
                }
            }
        }
        float s[U], mn = m;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float kf[8], a = 0.f;
            unpack(kr[u], kf);
#pragma unroll
            for (int i = 0; i < 8; ++i) a = fmaf(qf[i], kf[i], a);
#pragma unroll
            for (int off = G >> 1; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
            s[u] = (base + u * S + slot < len) ? a : -INFINITY;
            mn = fmaxf(mn, s[u]);
        }
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);      // (mn == -inf only while the slot has seen no key)
        l *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] *= alpha;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float p = (s[u] == -INFINITY) ? 0.f : __expf(s[u] - mn);
            float vf[8];
            unpack(vr[u], vf);                           // zeros for a key past len: 0 * 0, never 0 * NaN
            l += p;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fmaf(p, vf[i], o[i]);
        }
        m = mn;
    }

    // one combine: the workgroup's maximum, every slot rescaled to it, then plain sums over the slots
    float M = wave_max(m);
    if (lane == 0) red_m[w] = M;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; ++i) M = fmaxf(M, red_m[i]);
    const float sc = (m == -INFINITY) ? 0.f : __expf(m - M);
    l *= sc;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] *= sc;
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {             // lanes of equal c are G apart
        l += __shfl_xor(l, off, 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += __shfl_xor(o[i], off, 64);
    }
    if (lane < G) {
        red[w][lane][0] = l;
#pragma unroll
        for (int i = 0; i < 8; ++i) red[w][lane][1 + i] = o[i];
    }
    __syncthreads();
    if (tid < G && live) {
        float lt = 0.f, of[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) of[i] = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            lt += red[ww][tid][0];
#pragma unroll
            for (int i = 0; i < 8; ++i) of[i] += red[ww][tid][1 + i];
        }
        const float inv = 1.f / lt;
#pragma unroll
        for (int i = 0; i < 8; ++i) of[i] *= inv;
        st8<T>(out + (int64_t)b * ldo + col, of);
    }
}

// (value, index) order of torch.argmax: larger value first, NaN above everything, lower index on ties
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;
}

template <typename T>
__global__ __launch_bounds__(NT) void greedy_next_kernel(const T* __restrict__ logits, int64_t ldl,
                                                         const float* __restrict__ dict, const float* __restrict__ pe,
                                                         int64_t* __restrict__ tok, int64_t tok_stride, T* __restrict__ x,
                                                         int64_t ldx, int V, int D) {
    __shared__ float rv[NW];
    __shared__ int ri[NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t b = blockIdx.x;
    const T* row = logits + b * ldl;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += NT) {
        const float v = ld<T>(row + i);
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[w] = bv; ri[w] = bi; }
    __syncthreads();
    bv = rv[0];
    bi = ri[0];
#pragma unroll
    for (int i = 1; i < NW; ++i)
        if (better(rv[i], ri[i], bv, bi)) { bv = rv[i]; bi = ri[i]; }
    if (tid == 0) tok[b * tok_stride] = bi;
    const float* e = dict + (int64_t)bi * D;
    for (int i = tid; i < D; i += NT) st<T>(x + b * ldx + i, e[i] + pe[i]);
}

template <typename T>
void launch_decode(int G, dim3 grid, hipStream_t s, const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ldn,
                   void* kc, void* vc, int64_t ldc, int64_t bsc, void* out, int64_t ldo, int heads, int d, int len, float scale) {
#define FOCUS_DECODE_LAUNCH(LG)                                                                                              \
    hipLaunchKernelGGL((decode_attn_kernel<T, LG>), grid, dim3(NT), 0, s, (const T*)q, ldq, (const T*)k_new, (const T*)v_new, \
                       ldn, (T*)kc, (T*)vc, ldc, bsc, (T*)out, ldo, heads, d, len, scale)
    if (G == 1) FOCUS_DECODE_LAUNCH(0);
    else if (G == 2) FOCUS_DECODE_LAUNCH(1);
    else if (G == 4) FOCUS_DECODE_LAUNCH(2);
    else FOCUS_DECODE_LAUNCH(3);
#undef FOCUS_DECODE_LAUNCH
}

}  // namespace

extern "C" int focus_decode_attn_ok(int Lmax, int d, int dtype) {
    return (dtype == FOCUS_F32 || dtype == FOCUS_BF16) && d >= 8 && d <= 64 && d % 8 == 0 && Lmax >= 1 && Lmax <= (1 << 20);
}

extern "C" int focus_decode_attn(const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ldn, void* k_cache,
                                 void* v_cache, int64_t ldc, int64_t bsc, void* out, int64_t ldo, int B, int heads, int d, int len,
                                 int Lmax, float scale, int dtype, void* stream) {
    if (!q || !k_cache || !v_cache || !out) return FOCUS_ERR_NULL;
    if ((k_new == nullptr) != (v_new == nullptr)) return FOCUS_ERR_NULL;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (B < 1 || heads < 1 || d < 1 || len < 1 || len > Lmax || !focus_decode_attn_ok(Lmax, d, dtype)) return FOCUS_ERR_SHAPE;
    const int64_t C = (int64_t)heads * d;
    if ((int64_t)B * heads > 0x7fffffff) return FOCUS_ERR_SHAPE;
    const int64_t va = 16 / (int64_t)focus_esize(dtype);        // elements of a 16-byte access
    if (ldq < C || ldc < C || ldo < C || (k_new && ldn < C) || (B > 1 && bsc < (int64_t)(Lmax - 1) * ldc + C)) return FOCUS_ERR_ALIGN;
    if (ldq % va || ldc % va || ldo % va || bsc % va || (k_new && ldn % va)) return FOCUS_ERR_ALIGN;
    if (!focus_aligned(q, 16) || !focus_aligned(k_cache, 16) || !focus_aligned(v_cache, 16) || !focus_aligned(out, 16) ||
        !focus_aligned(k_new, 16) || !focus_aligned(v_new, 16))
        return FOCUS_ERR_ALIGN;
    const int chunks = d / 8;
    const int G = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 8;
    const dim3 grid((unsigned)(B * heads));
    if (dtype == FOCUS_BF16)
        launch_decode<bf16_t>(G, grid, (hipStream_t)stream, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, bsc, out, ldo, heads,
                              d, len, scale);
    else
        launch_decode<float>(G, grid, (hipStream_t)stream, q, ldq, k_new, v_new, ldn, k_cache, v_cache, ldc, bsc, out, ldo, heads, d,
                             len, scale);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_greedy_next(const void* logits, int64_t ldl, const float* dict, const float* pe_row, int64_t* tok,
                                 int64_t tok_stride, void* x_next, int64_t ldx, int B, int V, int D, int dtype, void* stream) {
    if (!logits || !dict || !pe_row || !tok || !x_next) return FOCUS_ERR_NULL;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (B < 1 || V < 1 || D < 1 || tok_stride < 1) return FOCUS_ERR_SHAPE;
    if (ldl < V || ldx < D) return FOCUS_ERR_ALIGN;
    if (!focus_aligned(logits, focus_esize(dtype)) || !focus_aligned(x_next, focus_esize(dtype)) || !focus_aligned(dict, 4) ||
        !focus_aligned(pe_row, 4) || !focus_aligned(tok, 8))
        return FOCUS_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        hipLaunchKernelGGL((greedy_next_kernel<bf16_t>), dim3((unsigned)B), dim3(NT), 0, s, (const bf16_t*)logits, ldl, dict, pe_row,
                           tok, tok_stride, (bf16_t*)x_next, ldx, V, D);
    else
        hipLaunchKernelGGL((greedy_next_kernel<float>), dim3((unsigned)B), dim3(NT), 0, s, (const float*)logits, ldl, dict, pe_row,
                           tok, tok_stride, (float*)x_next, ldx, V, D);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
