// batchnorm.hip -- BatchNorm2d (training statistics, apply, backward) and MaxPool2d(3, 2, 1) over channels-last maps.
// Every tensor is a row matrix [R, C] (R = N*H*W, row stride C, C % 8 == 0, C <= 256).  A thread owns 8 consecutive
// channels (one 16-byte access for bf16, two for fp32); a 256-thread workgroup is RPB = 256 / (C/8) row lanes x C/8 channel
// groups and walks the rows grid-stride, 4 rows' loads in flight per thread.  All of it is HBM-bound: the statistics read x
// once, the apply reads x (+ residual) and writes y, the backward reads dy, x (+ y) twice and writes dx (+ dres).
// Reductions over the rows are two-stage in a fixed order (block partials in a caller-owned workspace, no atomics).
#include "focus_common.h"
#include <algorithm>

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_BLOCKS = 1024;   // reductions: block partials the finish kernels walk (4 workgroups per CU)
constexpr int BN_UN = 4;              // rows in flight per thread

// (count, mean, M2) of a set merged with those of another (Chan et al.): exact in the counts, no E[x^2] - E[x]^2.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    if (nb == 0.f) return;
    const float n = na + nb, d = mb - ma, f = nb / n;
    ma += d * f;
    qa += qb + d * d * (na * f);
    na = n;
}

// Stage 1 of the statistics: every thread runs Welford's update over its rows, the row lanes of the workgroup are merged
// through LDS in lane order, the workgroup's (mean, M2) rows go to pmean / pm2 [nblk][C] and its count to pcnt[nblk].
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial(const T* __restrict__ x, float* __restrict__ pmean,
                                                                float* __restrict__ pm2, float* __restrict__ pcnt,
                                                                int64_t R, int C) {
    __shared__ float sm[17][BN_THREADS];
    const int CG = C >> 3, RPB = BN_THREADS / CG;
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
    float mean[8], m2[8], n = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { mean[e] = 0.f; m2[e] = 0.f; }
    if (rl < RPB) {
        const int64_t stride = (int64_t)gridDim.x * RPB;
        const T* xc = x + cg * 8;
        for (int64_t r0 = (int64_t)blockIdx.x * RPB + rl; r0 < R; r0 += BN_UN * stride) {
            float v[BN_UN][8];
#pragma unroll
            for (int u = 0; u < BN_UN; ++u) {
                const int64_t r = r0 + u * stride;
                ld8<T>(xc + (r < R ? r : r0) * C, v[u]);
            }
#pragma unroll
            for (int u = 0; u < BN_UN; ++u) {
                if (r0 + u * stride < R) {
                    n += 1.f;
                    const float inv = 1.f / n;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = v[u][e] - mean[e];
                        mean[e] += d * inv;
                        m2[e] += d * (v[u][e] - mean[e]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { sm[e][threadIdx.x] = mean[e]; sm[8 + e][threadIdx.x] = m2[e]; }
    sm[16][threadIdx.x] = n;
    __syncthreads();
    if (rl == 0) {
        for (int j = 1; j < RPB; ++j) {
            const int t = j * CG + cg;
            const float nb = sm[16][t];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float ne = n;                                       // (the 8 channels share the counts)
                chan_merge(ne, mean[e], m2[e], nb, sm[e][t], sm[8 + e][t]);
            }
            n += nb;
        }
        st8<float>(pmean + (int64_t)blockIdx.x * C + cg * 8, mean);
        st8<float>(pm2 + (int64_t)blockIdx.x * C + cg * 8, m2);
        if (cg == 0) pcnt[blockIdx.x] = n;
    }
}

// Stage 2: one wave per channel.  Lane l merges partials l, l + 64, ... in that order, then a 6-step tree over the lanes
// (lane l takes lane l + o); lane 0 holds the channel's (R, mean, M2).
__global__ __launch_bounds__(BN_THREADS) void bn_stats_finish(const float* __restrict__ pmean, const float* __restrict__ pm2,
                                                               const float* __restrict__ pcnt, float* __restrict__ mean,
                                                               float* __restrict__ rstd, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, int nblk, int C, float fR,
                                                               float fRm1, float eps, float momentum) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    float n = 0.f, m = 0.f, q = 0.f;
    for (int k = lane; k < nblk; k += 64) chan_merge(n, m, q, pcnt[k], pmean[(int64_t)k * C + c], pm2[(int64_t)k * C + c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float nb = __shfl_down(n, o, 64), mb = __shfl_down(m, o, 64), qb = __shfl_down(q, o, 64);
        chan_merge(n, m, q, nb, mb, qb);
    }
    if (lane == 0) {
        mean[c] = m;
        rstd[c] = 1.f / sqrtf(q / fR + eps);
        if (running_mean) {
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (q / fRm1);
        }
    }
}

// y = act(gamma (x - mean) rstd + beta [+ residual])
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const T* __restrict__ res,
                                                               T* __restrict__ y, int64_t R, int C) {
    const int CG = C >> 3, RPB = BN_THREADS / CG;
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
    if (rl >= RPB) return;
    float mu[8], s[8], b[8];
    ld8<float>(mean + cg * 8, mu);
    ld8<float>(rstd + cg * 8, s);
    ld8<float>(gamma + cg * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] *= b[e];
    ld8<float>(beta + cg * 8, b);
    const int64_t stride = (int64_t)gridDim.x * RPB;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB + rl; r0 < R; r0 += BN_UN * stride) {
        float v[BN_UN][8], rv[BN_UN][8];
#pragma unroll
        for (int u = 0; u < BN_UN; ++u) {
            const int64_t r = r0 + u * stride, rr = r < R ? r : r0;
            ld8<T>(x + rr * C + cg * 8, v[u]);
            if (RES) ld8<T>(res + rr * C + cg * 8, rv[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_UN; ++u) {
            const int64_t r = r0 + u * stride;
            if (r < R) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    o[e] = (v[u][e] - mu[e]) * s[e] + b[e];
                    if (RES) o[e] += rv[u][e];
                    if (RELU) o[e] = o[e] < 0.f ? 0.f : o[e];          // (keeps a NaN, as torch.relu does)
                }
                st8<T>(y + r * C + cg * 8, o);
            }
        }
    }
}

// Backward, pass 1: the workgroup's sums of g x^ and g over its rows -> partial[0 | 1][blk][C].
template <typename T, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce(const T* __restrict__ dy, const T* __restrict__ x,
                                                             const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ partial,
                                                             int64_t R, int C) {
    __shared__ float sm[16][BN_THREADS];
    const int CG = C >> 3, RPB = BN_THREADS / CG;
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
    float sgx[8], sg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sgx[e] = 0.f; sg[e] = 0.f; }
    if (rl < RPB) {
        float mu[8], rs[8];
        ld8<float>(mean + cg * 8, mu);
        ld8<float>(rstd + cg * 8, rs);
        const int64_t stride = (int64_t)gridDim.x * RPB;
        for (int64_t r0 = (int64_t)blockIdx.x * RPB + rl; r0 < R; r0 += BN_UN * stride) {
            float g[BN_UN][8], v[BN_UN][8], yv[BN_UN][8];
#pragma unroll
            for (int u = 0; u < BN_UN; ++u) {
                const int64_t r = r0 + u * stride, rr = r < R ? r : r0;
                ld8<T>(dy + rr * C + cg * 8, g[u]);
                ld8<T>(x + rr * C + cg * 8, v[u]);
                if (RELU) ld8<T>(y + rr * C + cg * 8, yv[u]);
            }
#pragma unroll
            for (int u = 0; u < BN_UN; ++u) {
                if (r0 + u * stride < R) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float ge = RELU ? (yv[u][e] > 0.f ? g[u][e] : 0.f) : g[u][e];
                        sg[e] += ge;
                        sgx[e] += ge * ((v[u][e] - mu[e]) * rs[e]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { sm[e][threadIdx.x] = sgx[e]; sm[8 + e][threadIdx.x] = sg[e]; }
    __syncthreads();
    if (rl == 0) {
        for (int j = 1; j < RPB; ++j) {
            const int t = j * CG + cg;
#pragma unroll
            for (int e = 0; e < 8; ++e) { sgx[e] += sm[e][t]; sg[e] += sm[8 + e][t]; }
        }
        st8<float>(partial + (int64_t)blockIdx.x * C + cg * 8, sgx);
        st8<float>(partial + ((int64_t)gridDim.x + blockIdx.x) * C + cg * 8, sg);
    }
}

// grid (ceil(C/64), 2), 1024 threads = 64 columns x 16 row lanes; blockIdx.y selects dgamma / dbeta (as ln_bwd_finish).
__global__ __launch_bounds__(1024) void bn_bwd_finish(const float* __restrict__ partial, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, int nblk, int C) {
    __shared__ float red[16][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const float* p = partial + (int64_t)blockIdx.y * nblk * C;
    float a = 0.f;
    if (c < C) {
#pragma unroll 8
        for (int k = rl; k < nblk; k += 16) a += p[(int64_t)k * C + c];
    }
    red[rl][cl] = a;
    __syncthreads();
    if (rl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        (blockIdx.y == 0 ? dgamma : dbeta)[c] = t;
    }
}

// Backward, pass 2: dx = gamma rstd (g - dbeta / R - x^ dgamma / R)  (frozen: gamma rstd g), dres = g.
template <typename T, bool RELU, bool DRES>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_dx(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                         const float* __restrict__ dbeta, T* __restrict__ dx,
                                                         T* __restrict__ dres, int64_t R, int C, int frozen, float invR) {
    const int CG = C >> 3, RPB = BN_THREADS / CG;
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
    if (rl >= RPB) return;
    float mu[8], rs[8], a[8], k1[8], k2[8];
    ld8<float>(mean + cg * 8, mu);
    ld8<float>(rstd + cg * 8, rs);
    ld8<float>(gamma + cg * 8, a);
    ld8<float>(dbeta + cg * 8, k1);
    ld8<float>(dgamma + cg * 8, k2);
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] *= rs[e]; k1[e] *= invR; k2[e] *= invR; }
    const int64_t stride = (int64_t)gridDim.x * RPB;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB + rl; r0 < R; r0 += BN_UN * stride) {
        float g[BN_UN][8], v[BN_UN][8], yv[BN_UN][8];
#pragma unroll
        for (int u = 0; u < BN_UN; ++u) {
            const int64_t r = r0 + u * stride, rr = r < R ? r : r0;
            ld8<T>(dy + rr * C + cg * 8, g[u]);
            ld8<T>(x + rr * C + cg * 8, v[u]);
            if (RELU) ld8<T>(y + rr * C + cg * 8, yv[u]);
        }
#pragma unroll
        for (int u = 0; u < BN_UN; ++u) {
            const int64_t r = r0 + u * stride;
            if (r < R) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (RELU) g[u][e] = yv[u][e] > 0.f ? g[u][e] : 0.f;
                    o[e] = frozen ? a[e] * g[u][e] : a[e] * (g[u][e] - k1[e] - (v[u][e] - mu[e]) * rs[e] * k2[e]);
                }
                st8<T>(dx + r * C + cg * 8, o);
                if (DRES) st8<T>(dres + r * C + cg * 8, g[u]);
            }
        }
    }
}

// ---- MaxPool2d(3, 2, 1): a thread per (output pixel, 8 channels) ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                  int8_t* __restrict__ idx, int N, int H, int W, int C, int OH,
                                                                  int OW) {
    const int CG = C >> 3;
    const int64_t total = (int64_t)N * OH * OW * CG;
    for (int64_t i = (int64_t)blockIdx.x * BN_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * BN_THREADS) {
        const int cg = (int)(i % CG);
        int64_t p = i / CG;
        const int ow = (int)(p % OW);
        p /= OW;
        const int oh = (int)(p % OH);
        const int64_t n = p / OH;
        float best[8];
        int bi[8];
        bool first = true;                                          // (the window's centre is always inside the map)
#pragma unroll
        for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 4; }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int h = 2 * oh - 1 + kh;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int w = 2 * ow - 1 + kw;
                if (w < 0 || w >= W) continue;
                float v[8];
                ld8<T>(x + ((n * H + h) * W + w) * C + cg * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // the first position opens the window; later ones need to be larger (or a NaN): the first maximum wins
                    if (first || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = kh * 3 + kw; }
                }
                first = false;
            }
        }
        const int64_t o = ((n * OH + oh) * OW + ow) * C + cg * 8;
        st8<T>(y + o, best);
        uint2 pk;
        pk.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
        pk.y = (uint32_t)bi[4] | ((uint32_t)bi[5] << 8) | ((uint32_t)bi[6] << 16) | ((uint32_t)bi[7] << 24);
        *reinterpret_cast<uint2*>(idx + o) = pk;
    }
}

// A thread per (input pixel, 8 channels): the windows oh in [h/2, (h+1)/2], ow likewise cover it; row-major order.
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void maxpool_bwd_kernel(const T* __restrict__ dy, const int8_t* __restrict__ idx,
                                                                  T* __restrict__ dx, int N, int H, int W, int C, int OH,
                                                                  int OW) {
    const int CG = C >> 3;
    const int64_t total = (int64_t)N * H * W * CG;
    for (int64_t i = (int64_t)blockIdx.x * BN_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * BN_THREADS) {
        const int cg = (int)(i % CG);
        int64_t p = i / CG;
        const int w = (int)(p % W);
        p /= W;
        const int h = (int)(p % H);
        const int64_t n = p / H;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        const int oh1 = min((h + 1) / 2, OH - 1), ow1 = min((w + 1) / 2, OW - 1);
        for (int oh = h / 2; oh <= oh1; ++oh) {
            for (int ow = w / 2; ow <= ow1; ++ow) {
                const uint32_t k = (uint32_t)((h - (2 * oh - 1)) * 3 + (w - (2 * ow - 1)));
                const int64_t o = ((n * OH + oh) * OW + ow) * C + cg * 8;
                float g[8];
                ld8<T>(dy + o, g);
                const uint2 pk = *reinterpret_cast<const uint2*>(idx + o);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t sel = ((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 0xffu;
                    acc[e] += sel == k ? g[e] : 0.f;
                }
            }
        }
        st8<T>(dx + ((n * H + h) * W + w) * C + cg * 8, acc);
    }
}

inline bool bn_c_ok(int C) { return C >= 8 && C <= 256 && (C & 7) == 0; }
inline bool bn_dtype_ok(int dtype) { return dtype == FOCUS_F32 || dtype == FOCUS_BF16; }
inline bool al16(const void* p) { return focus_aligned(p, 16); }      // (NULL is aligned)
inline int bn_rpb(int C) { return BN_THREADS / (C >> 3); }
inline int bn_apply_grid(int64_t R, int C) {
    return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(R, (int64_t)bn_rpb(C) * BN_UN), 1), 4096);
}

}  // namespace

extern "C" int focus_bn_blocks(int64_t R) {
    const int64_t b = cdiv64(R, 32);
    return (int)(b < 1 ? 1 : (b > BN_MAX_BLOCKS ? BN_MAX_BLOCKS : b));
}

// stats: mean, M2 [nblk][C] and the counts [nblk]; backward: partial [2][nblk][C]
extern "C" size_t focus_bn_workspace_bytes(int64_t R, int C) {
    if (!bn_c_ok(C) || R < 0) return 0;
    const size_t nblk = (size_t)focus_bn_blocks(R);
    return (nblk * (2 * (size_t)C + 1) * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" int focus_bn_stats(const void* x, float* mean, float* rstd, float* running_mean, float* running_var,
                              void* workspace, int64_t R, int C, float eps, float momentum, int dtype, void* stream) {
    if (!x || !mean || !rstd || !workspace || (!running_mean != !running_var)) return FOCUS_ERR_NULL;
    if (!bn_c_ok(C) || R < 2) return FOCUS_ERR_SHAPE;
    if (!bn_dtype_ok(dtype)) return FOCUS_ERR_DTYPE;
    if (!al16(x) || !al16(mean) || !al16(rstd) || !al16(running_mean) || !al16(running_var) || !al16(workspace))
        return FOCUS_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = focus_bn_blocks(R);
    float* pmean = (float*)workspace;
    float* pm2 = pmean + (size_t)nblk * C;
    float* pcnt = pm2 + (size_t)nblk * C;
    if (dtype == FOCUS_BF16)
        hipLaunchKernelGGL(bn_stats_partial<bf16_t>, dim3(nblk), dim3(BN_THREADS), 0, s, (const bf16_t*)x, pmean, pm2, pcnt, R, C);
    else
        hipLaunchKernelGGL(bn_stats_partial<float>, dim3(nblk), dim3(BN_THREADS), 0, s, (const float*)x, pmean, pm2, pcnt, R, C);
    FOCUS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_stats_finish, dim3(C / 4), dim3(BN_THREADS), 0, s, pmean, pm2, pcnt, mean, rstd, running_mean,
                       running_var, nblk, C, (float)R, (float)(R - 1), eps, momentum);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_bn_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                              const void* residual, void* y, int64_t R, int C, int relu, int dtype, void* stream) {
    // (an empty tensor has no address: with R == 0 the row-sized buffers may be NULL)
    if (!mean || !rstd || !gamma || !beta || (R > 0 && (!x || !y))) return FOCUS_ERR_NULL;
    if (!bn_c_ok(C) || R < 0) return FOCUS_ERR_SHAPE;
    if (!bn_dtype_ok(dtype)) return FOCUS_ERR_DTYPE;
    if (!al16(x) || !al16(y) || !al16(residual) || !al16(mean) || !al16(rstd) || !al16(gamma) || !al16(beta))
        return FOCUS_ERR_ALIGN;
    if (R == 0) return FOCUS_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(bn_apply_grid(R, C)), blk(BN_THREADS);
#define BN_APPLY(T, RELU, RES) hipLaunchKernelGGL((bn_apply_kernel<T, RELU, RES>), grid, blk, 0, s, (const T*)x, mean, rstd, gamma, beta, (const T*)residual, (T*)y, R, C)
#define BN_APPLY_T(T) do { if (relu) { if (residual) BN_APPLY(T, true, true); else BN_APPLY(T, true, false); } \
                           else { if (residual) BN_APPLY(T, false, true); else BN_APPLY(T, false, false); } } while (0)
    if (dtype == FOCUS_BF16) BN_APPLY_T(bf16_t); else BN_APPLY_T(float);
#undef BN_APPLY_T
#undef BN_APPLY
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_bn_bwd(const void* dy, const void* x, const void* y, const float* mean, const float* rstd,
                            const float* gamma, void* dx, void* dres, float* dgamma, float* dbeta, void* workspace, int64_t R,
                            int C, int relu, int frozen, int dtype, void* stream) {
    if (!mean || !rstd || !gamma || !dgamma || !dbeta || !workspace || (R > 0 && (!dy || !x || !dx || (relu && !y))))
        return FOCUS_ERR_NULL;
    if (!bn_c_ok(C) || R < 0) return FOCUS_ERR_SHAPE;
    if (!bn_dtype_ok(dtype)) return FOCUS_ERR_DTYPE;
    if (!al16(dy) || !al16(x) || !al16(y) || !al16(dx) || !al16(dres) || !al16(mean) || !al16(rstd) || !al16(gamma) ||
        !al16(dgamma) || !al16(dbeta) || !al16(workspace))
        return FOCUS_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {                                                   // no rows: zero gradients
        if (hipMemsetAsync(dgamma, 0, (size_t)C * sizeof(float), s) != hipSuccess ||
            hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), s) != hipSuccess)
            return FOCUS_ERR_LAUNCH;
        return FOCUS_OK;
    }
    const int nblk = focus_bn_blocks(R);
    float* partial = (float*)workspace;
    const dim3 blk(BN_THREADS), grid(bn_apply_grid(R, C));
    const float invR = (float)(1.0 / (double)R);
#define BN_RED(T, RELU) hipLaunchKernelGGL((bn_bwd_reduce<T, RELU>), dim3(nblk), blk, 0, s, (const T*)dy, (const T*)x, (const T*)y, mean, rstd, partial, R, C)
#define BN_DX(T, RELU, DRES) hipLaunchKernelGGL((bn_bwd_dx<T, RELU, DRES>), grid, blk, 0, s, (const T*)dy, (const T*)x, (const T*)y, mean, rstd, gamma, dgamma, dbeta, (T*)dx, (T*)dres, R, C, frozen, invR)
#define BN_BWD_T(T) do { \
        if (relu) BN_RED(T, true); else BN_RED(T, false); \
        FOCUS_CHECK_LAUNCH(); \
        hipLaunchKernelGGL(bn_bwd_finish, dim3((C + 63) / 64, 2), dim3(1024), 0, s, partial, dgamma, dbeta, nblk, C); \
        FOCUS_CHECK_LAUNCH(); \
        if (relu) { if (dres) BN_DX(T, true, true); else BN_DX(T, true, false); } \
        else { if (dres) BN_DX(T, false, true); else BN_DX(T, false, false); } } while (0)
    if (dtype == FOCUS_BF16) BN_BWD_T(bf16_t); else BN_BWD_T(float);
#undef BN_BWD_T
#undef BN_DX
#undef BN_RED
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

static int pool_check(const void* a, const void* b, const void* c, int N, int H, int W, int C, int dtype) {
    if (N > 0 && (!a || !b || !c)) return FOCUS_ERR_NULL;
    if (!bn_c_ok(C) || N < 0 || H < 1 || W < 1 || (int64_t)N * H * W >= ((int64_t)1 << 31)) return FOCUS_ERR_SHAPE;
    if (!bn_dtype_ok(dtype)) return FOCUS_ERR_DTYPE;
    if (!al16(a) || !al16(b) || !al16(c)) return FOCUS_ERR_ALIGN;
    return FOCUS_OK;
}

extern "C" int focus_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int dtype, void* stream) {
    const int rc = pool_check(x, y, idx, N, H, W, C, dtype);
    if (rc != FOCUS_OK || N == 0) return rc;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)N * OH * OW * (C >> 3);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv64(total, BN_THREADS), 8192)), blk(BN_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        hipLaunchKernelGGL(maxpool_fwd_kernel<bf16_t>, grid, blk, 0, s, (const bf16_t*)x, (bf16_t*)y, (int8_t*)idx, N, H, W, C, OH, OW);
    else
        hipLaunchKernelGGL(maxpool_fwd_kernel<float>, grid, blk, 0, s, (const float*)x, (float*)y, (int8_t*)idx, N, H, W, C, OH, OW);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_maxpool_bwd(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, int dtype,
                                 void* stream) {
    const int rc = pool_check(dy, idx, dx, N, H, W, C, dtype);
    if (rc != FOCUS_OK || N == 0) return rc;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)N * H * W * (C >> 3);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv64(total, BN_THREADS), 8192)), blk(BN_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        hipLaunchKernelGGL(maxpool_bwd_kernel<bf16_t>, grid, blk, 0, s, (const bf16_t*)dy, (const int8_t*)idx, (bf16_t*)dx, N, H, W, C, OH, OW);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<float>, grid, blk, 0, s, (const float*)dy, (const int8_t*)idx, (float*)dx, N, H, W, C, OH, OW);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
