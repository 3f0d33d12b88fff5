// token_pool.hip -- the pooling operators of MViT's pooling attention (attention.py:16-50: depth-wise Conv3d, MaxPool3d,
// AvgPool3d over the (T, H, W) grid) in token layout, with the per-head LayerNorm that follows them fused into the forward.
// Every tensor is a row matrix [B, cls + T*H*W, C] with heads as column blocks of head_dim: pooling reads neighbouring rows,
// the depth-wise weight of column c is w[c % head_dim], the LayerNorm runs over head_dim-wide column groups.  A lane owns 8
// consecutive channels (one 16-byte access for bf16, two for fp32); arithmetic is fp32.  All of it is memory-bound: window
// reuse is left to L2, the grids are capped at 2048 workgroups and grid-stride the rest.
//   forward   a lane per (output row, 8 channels).  With the LayerNorm a column group takes G = head_dim / 8 lanes padded to
//             the next power of two (12 -> 16 for head_dim 96) so that its two sums are xor-shuffles inside the wave.
//   dx        a gather: a lane per (input row, 8 channels) walks the output positions whose window covers its cell.
//   dw        two stages in a fixed order (no atomics): a lane accumulates 9 taps x 8 channels over its output rows, a
//             workgroup folds its row lanes and heads through LDS into partial[block][head_dim][taps]; one pass sums them.
// The conv weights [head_dim, taps] are staged in LDS as [taps][head_dim] when they fit 32 KiB, else read from memory.
#include "focus_common.h"
#include <algorithm>

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_MAX_BLOCKS = 2048;      // forward and dx grids
constexpr int TP_DW_MAX_BLOCKS = 256;    // row blocks of the dw partials
constexpr int TP_DW_ROWS = 4;            // output rows a dw row lane takes before another row block is opened
constexpr int TP_TAPS = 9;               // taps a dw lane accumulates (9 x 8 fp32 accumulators)
constexpr int TP_WLDS_FLOATS = 8192;     // conv weights go through LDS when head_dim * taps <= this

enum { TP_CONV = FOCUS_POOL_CONV, TP_MAX = FOCUS_POOL_MAX, TP_AVG = FOCUS_POOL_AVG };

struct Geo {
    int B, T, H, W, C, hd, cls;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
    int OT, OH, OW, rows_in, rows_out;   // rows per sample, the cls row included
    int64_t xbs, xrs;
    int UG, UGP;                         // lanes of a forward unit and their padded count (1, 1 without the LayerNorm)
};

__device__ __forceinline__ void tp_w8(const float* wsm, const float* __restrict__ w, int wlds, int hd, int K, int wch, int tap,
                                      float (&o)[8]) {
    if (wlds) {
        ld8<float>(wsm + tap * hd + wch, o);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = w[(wch + e) * K + tap];
    }
}

__device__ __forceinline__ void tp_stage_weights(float* wsm, const float* __restrict__ w, int hd, int K) {
    for (int i = threadIdx.x; i < hd * K; i += TP_THREADS) wsm[(i % K) * hd + i / K] = w[i];
    __syncthreads();
}

__device__ __forceinline__ int tp_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- forward ---------------------------------------------------------------------------------------------------------
// KT == 0: the window extents are read from the descriptor (the generic loop).
template <typename T, int MODE, int KT, int KH, int KW>
__global__ __launch_bounds__(TP_THREADS) void tp_fwd_kernel(Geo g, const T* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float eps, T* __restrict__ y, T* __restrict__ pooled,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int8_t* __restrict__ idx, int wlds) {
    extern __shared__ float tp_wsm[];
    const int kt = KT ? KT : g.kt, kh = KT ? KH : g.kh, kw = KT ? KW : g.kw;
    const int K = kt * kh * kw;
    if (MODE == TP_CONV && wlds) tp_stage_weights(tp_wsm, w, g.hd, K);
    const int lg = threadIdx.x & (g.UGP - 1), ub = threadIdx.x / g.UGP, UPB = TP_THREADS / g.UGP;
    const bool act = lg < g.UG;
    const int upr = g.C / (8 * g.UG);                                   // units of a row
    // (B * rows * C < 2^31: every index below fits 32 bits, and 32-bit divisions are a quarter of the 64-bit ones)
    const uint32_t U = (uint32_t)g.B * g.rows_out * upr;
    for (uint32_t u = blockIdx.x * UPB + ub; u < U; u += gridDim.x * UPB) {
        const int uh = (int)(u % (uint32_t)upr);
        const uint32_t br = u / (uint32_t)upr;
        const int r = (int)(br % (uint32_t)g.rows_out);
        const int64_t b = br / (uint32_t)g.rows_out;
        const int col = (uh * g.UG + (act ? lg : 0)) * 8;               // (a padding lane reads with lane 0 and stores nothing)
        const int wch = col % g.hd;
        const T* xb = x + b * g.xbs + col;
        float v[8];
        int bi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[e] = 0.f; bi[e] = 0xff; }
        if (g.cls && r == 0) {
            ld8<T>(xb, v);
        } else {
            const int o = r - g.cls;
            const int ow = o % g.OW, oh = (o / g.OW) % g.OH, ot = o / (g.OW * g.OH);
            const int t0 = ot * g.st - g.pt, h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
            bool first = true;
#pragma unroll 1
            for (int a = 0; a < kt; ++a) {                              // (a kh x kw plane of loads in flight)
                const int t = t0 + a;
                const bool tin = t >= 0 && t < g.T;
                const int tc = tp_clamp(t, g.T);
#pragma unroll
                for (int bq = 0; bq < kh; ++bq) {
                    const int h = h0 + bq;
                    const bool hin = tin && h >= 0 && h < g.H;
                    const int hc = tp_clamp(h, g.H);
#pragma unroll
                    for (int c = 0; c < kw; ++c) {
                        const int wq = w0 + c;
                        const bool inb = hin && wq >= 0 && wq < g.W;
                        const int wc = tp_clamp(wq, g.W);
                        const int tap = (a * kh + bq) * kw + c;
                        float xv[8];
                        ld8<T>(xb + (int64_t)(g.cls + (tc * g.H + hc) * g.W + wc) * g.xrs, xv);      // (clamped: always inside)
                        if (MODE == TP_CONV) {
                            float wv[8];
                            tp_w8(tp_wsm, w, wlds, g.hd, K, wch, tap, wv);
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = fmaf(wv[e], inb ? xv[e] : 0.f, v[e]);
                        } else if (MODE == TP_AVG) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] += inb ? xv[e] : 0.f;
                        } else {
                            // the first in-bounds tap opens the window; later ones need to be larger (or a NaN)
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                if (inb && (first || xv[e] > v[e] || xv[e] != xv[e])) { v[e] = xv[e]; bi[e] = tap; }
                            if (inb) first = false;
                        }
                    }
                }
            }
            if (MODE == TP_AVG) {
                const float fk = (float)K;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = v[e] / fk;
            }
        }
        const int64_t off = (b * g.rows_out + r) * g.C + col;
        if (MODE == TP_MAX && act) {
            uint2 pk;
            pk.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
            pk.y = (uint32_t)bi[4] | ((uint32_t)bi[5] << 8) | ((uint32_t)bi[6] << 16) | ((uint32_t)bi[7] << 24);
            *reinterpret_cast<uint2*>(idx + off) = pk;
        }
        if (gamma == nullptr) {
            if (act) st8<T>(y + off, v);
            continue;
        }
        // LayerNorm over the head_dim columns of the unit, from the un-rounded fp32 values: two passes, biased variance
        float s = 0.f;
        if (act) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[e];
        }
        for (int o2 = g.UGP >> 1; o2 > 0; o2 >>= 1) s += __shfl_xor(s, o2, 64);
        const float fd = (float)g.hd;
        const float mu = s / fd;
        float d[8], q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { d[e] = v[e] - mu; q += d[e] * d[e]; }
        if (!act) q = 0.f;
        for (int o2 = g.UGP >> 1; o2 > 0; o2 >>= 1) q += __shfl_xor(q, o2, 64);
        const float rs = 1.f / sqrtf(q / fd + eps);
        if (act) {
            float ga[8], be[8], out[8];
            ld8<float>(gamma + wch, ga);
            ld8<float>(beta + wch, be);
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] = d[e] * rs * ga[e] + be[e];
            st8<T>(y + off, out);
            if (pooled) {                                               // (not kept for an inference-only forward)
                st8<T>(pooled + off, v);
                if (lg == 0) { mean[u] = mu; rstd[u] = rs; }
            }
        }
    }
}

// ---- dx: a lane per (input row, 8 channels) ----------------------------------------------------------------------------
// The output positions o with 0 <= i + p - o s < k cover cell i; the tap is i + p - o s.
__device__ __forceinline__ void tp_cover(int i, int p, int k, int s, int O, int& lo, int& hi) {
    const int n = i + p;
    hi = min(n / s, O - 1);
    const int m = n - k + 1;
    lo = m <= 0 ? 0 : (m + s - 1) / s;
}

template <typename T, int MODE>
__global__ __launch_bounds__(TP_THREADS) void tp_dx_kernel(Geo g, const T* __restrict__ dp, const float* __restrict__ w,
                                                           const int8_t* __restrict__ idx, T* __restrict__ dx, int wlds) {
    extern __shared__ float tp_wsm[];
    const int K = g.kt * g.kh * g.kw;
    if (MODE == TP_CONV && wlds) tp_stage_weights(tp_wsm, w, g.hd, K);
    const int CG = g.C >> 3;
    const uint32_t total = (uint32_t)g.B * g.rows_in * CG;             // (< 2^31, as in the forward)
    for (uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x; i < total; i += gridDim.x * TP_THREADS) {
        const int cg = (int)(i % (uint32_t)CG);
        const uint32_t br = i / (uint32_t)CG;
        const int r = (int)(br % (uint32_t)g.rows_in);
        const int64_t b = br / (uint32_t)g.rows_in;
        const int col = cg * 8, wch = col % g.hd;
        const T* dpb = dp + b * g.rows_out * g.C + col;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        if (g.cls && r == 0) {
            ld8<T>(dpb, acc);
        } else {
            const int cell = r - g.cls;
            const int wi = cell % g.W, hi_ = (cell / g.W) % g.H, ti = cell / (g.W * g.H);
            int t_lo, t_hi, h_lo, h_hi, w_lo, w_hi;
            tp_cover(ti, g.pt, g.kt, g.st, g.OT, t_lo, t_hi);
            tp_cover(hi_, g.ph, g.kh, g.sh, g.OH, h_lo, h_hi);
            tp_cover(wi, g.pw, g.kw, g.sw, g.OW, w_lo, w_hi);
            for (int ot = t_lo; ot <= t_hi; ++ot) {
                const int a = ti + g.pt - ot * g.st;
                for (int oh = h_lo; oh <= h_hi; ++oh) {
                    const int bq = hi_ + g.ph - oh * g.sh;
                    for (int ow = w_lo; ow <= w_hi; ++ow) {
                        const int c = wi + g.pw - ow * g.sw;
                        const int tap = (a * g.kh + bq) * g.kw + c;
                        const int64_t o = (int64_t)(g.cls + (ot * g.OH + oh) * g.OW + ow) * g.C;
                        float gv[8];
                        ld8<T>(dpb + o, gv);
                        if (MODE == TP_CONV) {
                            float wv[8];
                            tp_w8(tp_wsm, w, wlds, g.hd, K, wch, tap, wv);
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wv[e], gv[e], acc[e]);
                        } else if (MODE == TP_AVG) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[e] += gv[e];
                        } else {
                            const uint2 pk = *reinterpret_cast<const uint2*>(idx + b * g.rows_out * g.C + col + o);
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const uint32_t sel = ((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 0xffu;
                                acc[e] += sel == (uint32_t)tap ? gv[e] : 0.f;
                            }
                        }
                    }
                }
            }
            if (MODE == TP_AVG) {
                const float fk = (float)K;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = acc[e] / fk;
            }
        }
        st8<T>(dx + (b * g.rows_in + r) * g.C + col, acc);
    }
}

// ---- dw, stage 1: grid (row blocks, tap chunks, channel-group tiles) ---------------------------------------------------
// Thread (rl, cgl): row lane rl of RL = 256 / CGW, channel group blockIdx.z * CGW + cgl.  partial[z][x][head_dim][taps].
template <typename T>
__global__ __launch_bounds__(TP_THREADS) void tp_dw_partial(Geo g, const T* __restrict__ dp, const T* __restrict__ x,
                                                            float* __restrict__ partial, int CGW, int RL) {
    __shared__ float sm[8][TP_THREADS];
    const int K = g.kt * g.kh * g.kw, CG = g.C >> 3, G = g.hd >> 3;
    const int cgl = threadIdx.x % CGW, rl = threadIdx.x / CGW;
    const int cg0 = blockIdx.z * CGW, cg = cg0 + cgl;
    const bool act = rl < RL && cg < CG;
    const int tap0 = blockIdx.y * TP_TAPS;
    int da[TP_TAPS], db[TP_TAPS], dc[TP_TAPS];
    bool tv[TP_TAPS];
#pragma unroll
    for (int j = 0; j < TP_TAPS; ++j) {
        const int tap = tap0 + j;
        tv[j] = tap < K;
        const int tt = tv[j] ? tap : 0;
        dc[j] = tt % g.kw;
        db[j] = (tt / g.kw) % g.kh;
        da[j] = tt / (g.kw * g.kh);
    }
    float acc[TP_TAPS][8];
#pragma unroll
    for (int j = 0; j < TP_TAPS; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    if (act) {
        const int OL = g.OT * g.OH * g.OW;
        const uint32_t R = (uint32_t)g.B * OL;
        for (uint32_t r = blockIdx.x * RL + rl; r < R; r += gridDim.x * RL) {
            const int o = (int)(r % (uint32_t)OL);
            const int64_t b = r / (uint32_t)OL;
            const int ow = o % g.OW, oh = (o / g.OW) % g.OH, ot = o / (g.OW * g.OH);
            float gv[8];
            ld8<T>(dp + (b * g.rows_out + g.cls + o) * g.C + cg * 8, gv);
            const T* xb = x + b * g.xbs + cg * 8;
#pragma unroll
            for (int j = 0; j < TP_TAPS; ++j) {
                if (!tv[j]) continue;
                const int t = ot * g.st - g.pt + da[j], h = oh * g.sh - g.ph + db[j], wq = ow * g.sw - g.pw + dc[j];
                const bool inb = t >= 0 && t < g.T && h >= 0 && h < g.H && wq >= 0 && wq < g.W;
                float xv[8];
                ld8<T>(xb + (int64_t)(g.cls + (tp_clamp(t, g.T) * g.H + tp_clamp(h, g.H)) * g.W + tp_clamp(wq, g.W)) * g.xrs, xv);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(gv[e], inb ? xv[e] : 0.f, acc[j][e]);
            }
        }
    }
    // the workgroup's row lanes and heads, one tap at a time: channel c = threadIdx.x sums the lanes that hold it, in order
    const int c = threadIdx.x, gl = c >> 3, ce = c & 7;
    const int first = ((gl - cg0 % G) % G + G) % G;
    float* out = partial + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * g.hd * K;
#pragma unroll
    for (int j = 0; j < TP_TAPS; ++j) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) sm[e][threadIdx.x] = act ? acc[j][e] : 0.f;
        __syncthreads();
        if (c < g.hd && tv[j]) {
            float s = 0.f;
            for (int k = first; k < CGW && cg0 + k < CG; k += G)
                for (int q = 0; q < RL; ++q) s += sm[ce][q * CGW + k];
            out[c * K + tap0 + j] = s;
        }
    }
}

// Stage 2: 1024 threads = 64 elements x 16 lanes; lane l sums partials l, l + 16, ..., then the 16 lanes in order.
__global__ __launch_bounds__(1024) void tp_dw_finish(const float* __restrict__ partial, float* __restrict__ dw, int NP, int n) {
    __shared__ float red[16][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + cl;
    float a = 0.f;
    if (i < n) {
#pragma unroll 8
        for (int k = rl; k < NP; k += 16) a += partial[(int64_t)k * n + i];
    }
    red[rl][cl] = a;
    __syncthreads();
    if (rl == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        dw[i] = t;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return focus_aligned(p, 16); }      // (NULL is aligned)
inline int pow2_up(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// SHAPE / DTYPE of a descriptor, and its geometry.  norm: the forward normalises (groups of head_dim columns).
int tp_geo(const focus_token_pool_desc* d, bool norm, Geo& g) {
    if (d->B < 0 || d->T < 1 || d->H < 1 || d->W < 1 || d->C < 8 || d->C > 4096 || d->head_dim < 8 || (d->head_dim & 7) ||
        d->C % d->head_dim || (d->cls != 0 && d->cls != 1) || d->mode < TP_CONV || d->mode > TP_AVG)
        return FOCUS_ERR_SHAPE;
    int o[3];
    const int in[3] = {d->T, d->H, d->W};
    for (int i = 0; i < 3; ++i) {
        if (d->k[i] < 1 || d->k[i] > 7 || d->s[i] < 1 || d->s[i] > 8 || d->p[i] < 0 || d->p[i] >= d->k[i]) return FOCUS_ERR_SHAPE;
        const int n = in[i] + 2 * d->p[i] - d->k[i];
        if (n < 0) return FOCUS_ERR_SHAPE;
        o[i] = n / d->s[i] + 1;
    }
    if ((norm || d->mode == TP_CONV) && d->head_dim > 128) return FOCUS_ERR_SHAPE;
    if (d->mode == TP_MAX && d->k[0] * d->k[1] * d->k[2] > 127) return FOCUS_ERR_SHAPE;      // the tap is stored in an int8
    const int64_t rows_in = d->cls + (int64_t)d->T * d->H * d->W, rows_out = d->cls + (int64_t)o[0] * o[1] * o[2];
    const int64_t lim = (int64_t)1 << 31;
    if (rows_in >= lim || rows_out >= lim || d->B * rows_in * d->C >= lim || d->B * rows_out * d->C >= lim) return FOCUS_ERR_SHAPE;
    if (d->x_row_stride < d->C || d->x_batch_stride < 0) return FOCUS_ERR_SHAPE;
    if (d->dtype != FOCUS_F32 && d->dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    g.B = d->B; g.T = d->T; g.H = d->H; g.W = d->W; g.C = d->C; g.hd = d->head_dim; g.cls = d->cls;
    g.kt = d->k[0]; g.kh = d->k[1]; g.kw = d->k[2];
    g.st = d->s[0]; g.sh = d->s[1]; g.sw = d->s[2];
    g.pt = d->p[0]; g.ph = d->p[1]; g.pw = d->p[2];
    g.OT = o[0]; g.OH = o[1]; g.OW = o[2];
    g.rows_in = (int)rows_in; g.rows_out = (int)rows_out;
    g.xbs = d->x_batch_stride; g.xrs = d->x_row_stride;
    g.UG = norm ? d->head_dim >> 3 : 1;
    g.UGP = pow2_up(g.UG);
    return FOCUS_OK;
}

inline bool tp_strides_aligned(const focus_token_pool_desc* d) {
    const int64_t a = 16 / (int64_t)focus_esize(d->dtype);
    return d->x_row_stride % a == 0 && d->x_batch_stride % a == 0;
}

inline int tp_fwd_grid(const Geo& g) {
    const int64_t lanes = (int64_t)g.B * g.rows_out * (g.C / (8 * g.UG)) * g.UGP;
    return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(lanes, TP_THREADS), 1), TP_MAX_BLOCKS);
}
inline int tp_dx_grid(const Geo& g) {
    const int64_t lanes = (int64_t)g.B * g.rows_in * (g.C >> 3);
    return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(lanes, TP_THREADS), 1), TP_MAX_BLOCKS);
}
inline int tp_dw_cgw(const Geo& g) { return std::min(g.C >> 3, TP_THREADS); }
inline int tp_dw_tiles(const Geo& g) { return (int)cdiv64(g.C >> 3, tp_dw_cgw(g)); }
inline int tp_dw_rowblocks(const Geo& g) {
    const int RL = TP_THREADS / tp_dw_cgw(g);
    const int64_t R = (int64_t)g.B * g.OT * g.OH * g.OW;
    return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(R, (int64_t)RL * TP_DW_ROWS), 1), TP_DW_MAX_BLOCKS);
}
inline size_t tp_ws_bytes(const Geo& g) {
    const size_t n = (size_t)tp_dw_rowblocks(g) * tp_dw_tiles(g) * g.hd * g.kt * g.kh * g.kw * sizeof(float);
    return (n + 15) & ~(size_t)15;
}
inline int tp_wlds(const Geo& g) { return g.hd * g.kt * g.kh * g.kw <= TP_WLDS_FLOATS; }

}  // namespace

extern "C" int focus_token_pool_blocks(const focus_token_pool_desc* d, int stage) {
    Geo g;
    if (!d || stage < 0 || stage > 3 || tp_geo(d, stage == 1, g) != FOCUS_OK) return 0;
    return stage <= 1 ? tp_fwd_grid(g) : stage == 2 ? tp_dx_grid(g) : tp_dw_rowblocks(g);
}

extern "C" size_t focus_token_pool_workspace_bytes(const focus_token_pool_desc* d) {
    Geo g;
    if (!d || d->mode != TP_CONV || tp_geo(d, false, g) != FOCUS_OK) return 0;
    return tp_ws_bytes(g);
}

extern "C" int focus_token_pool_fwd(const focus_token_pool_desc* d, const void* x, const float* w, const float* gamma,
                                    const float* beta, float eps, void* y, void* pooled, float* mean, float* rstd, void* idx,
                                    void* stream) {
    if (!d) return FOCUS_ERR_NULL;
    const bool norm = gamma || beta;
    Geo g;
    const int rc = tp_geo(d, norm, g);
    if (rc != FOCUS_OK) return rc;
    if (g.B == 0) return FOCUS_OK;
    if (!x || !y || (d->mode == TP_CONV && !w) || (d->mode == TP_MAX && !idx) ||
        (norm && (!gamma || !beta)) || (pooled || mean || rstd) != (pooled && mean && rstd))
        return FOCUS_ERR_NULL;
    if (!al16(x) || !al16(y) || !al16(w) || !al16(idx) || !tp_strides_aligned(d) ||
        (norm && (!al16(gamma) || !al16(beta) || !al16(pooled) || !al16(mean) || !al16(rstd))))
        return FOCUS_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(tp_fwd_grid(g)), blk(TP_THREADS);
    const int wlds = d->mode == TP_CONV && tp_wlds(g);
    const size_t lds = wlds ? (size_t)g.hd * g.kt * g.kh * g.kw * sizeof(float) : 0;
    const int win = (g.kt == 3 && g.kh == 3 && g.kw == 3) ? 1 : (g.kt == 1 && g.kh == 3 && g.kw == 3) ? 2 : 0;
#define TP_FWD(T, MODE, KT, KH, KW) hipLaunchKernelGGL((tp_fwd_kernel<T, MODE, KT, KH, KW>), grid, blk, lds, s, g, (const T*)x, w, gamma, beta, eps, (T*)y, (T*)pooled, mean, rstd, (int8_t*)idx, wlds)
#define TP_FWD_W(T, MODE) do { if (win == 1) TP_FWD(T, MODE, 3, 3, 3); else if (win == 2) TP_FWD(T, MODE, 1, 3, 3); else TP_FWD(T, MODE, 0, 0, 0); } while (0)
#define TP_FWD_M(T) do { if (d->mode == TP_CONV) TP_FWD_W(T, TP_CONV); else if (d->mode == TP_MAX) TP_FWD_W(T, TP_MAX); else TP_FWD_W(T, TP_AVG); } while (0)
    if (d->dtype == FOCUS_BF16) TP_FWD_M(bf16_t); else TP_FWD_M(float);
#undef TP_FWD_M
#undef TP_FWD_W
#undef TP_FWD
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_token_pool_bwd(const focus_token_pool_desc* d, const void* dpooled, const void* x, const float* w,
                                    const void* idx, void* dx, float* dw, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (!d) return FOCUS_ERR_NULL;
    Geo g;
    const int rc = tp_geo(d, false, g);
    if (rc != FOCUS_OK) return rc;
    if (dw && d->mode != TP_CONV) return FOCUS_ERR_SHAPE;
    if (g.B == 0) return FOCUS_OK;
    if (!dpooled || (!dx && !dw) || (dx && d->mode == TP_CONV && !w) || (dx && d->mode == TP_MAX && !idx) ||
        (dw && (!x || !workspace)))
        return FOCUS_ERR_NULL;
    if (!al16(dpooled) || !al16(x) || !al16(w) || !al16(idx) || !al16(dx) || !al16(dw) || !al16(workspace) ||
        !tp_strides_aligned(d))
        return FOCUS_ERR_ALIGN;
    if (dw && workspace_bytes < tp_ws_bytes(g)) return FOCUS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(TP_THREADS);
    if (dx) {
        const dim3 grid(tp_dx_grid(g));
        const int wlds = d->mode == TP_CONV && tp_wlds(g);
        const size_t lds = wlds ? (size_t)g.hd * g.kt * g.kh * g.kw * sizeof(float) : 0;
#define TP_DX(T, MODE) hipLaunchKernelGGL((tp_dx_kernel<T, MODE>), grid, blk, lds, s, g, (const T*)dpooled, w, (const int8_t*)idx, (T*)dx, wlds)
#define TP_DX_M(T) do { if (d->mode == TP_CONV) TP_DX(T, TP_CONV); else if (d->mode == TP_MAX) TP_DX(T, TP_MAX); else TP_DX(T, TP_AVG); } while (0)
        if (d->dtype == FOCUS_BF16) TP_DX_M(bf16_t); else TP_DX_M(float);
#undef TP_DX_M
#undef TP_DX
        FOCUS_CHECK_LAUNCH();
    }
    if (dw) {
        const int K = g.kt * g.kh * g.kw, CGW = tp_dw_cgw(g), RL = TP_THREADS / CGW;
        const int nblk = tp_dw_rowblocks(g), tiles = tp_dw_tiles(g);
        const dim3 grid(nblk, (K + TP_TAPS - 1) / TP_TAPS, tiles);
        if (d->dtype == FOCUS_BF16)
            hipLaunchKernelGGL(tp_dw_partial<bf16_t>, grid, blk, 0, s, g, (const bf16_t*)dpooled, (const bf16_t*)x, (float*)workspace, CGW, RL);
        else
            hipLaunchKernelGGL(tp_dw_partial<float>, grid, blk, 0, s, g, (const float*)dpooled, (const float*)x, (float*)workspace, CGW, RL);
        FOCUS_CHECK_LAUNCH();
        const int n = g.hd * K;
        hipLaunchKernelGGL(tp_dw_finish, dim3((n + 63) / 64), dim3(1024), 0, s, (const float*)workspace, dw, nblk * tiles, n);
        FOCUS_CHECK_LAUNCH();
    }
    return FOCUS_OK;
}
