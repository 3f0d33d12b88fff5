// randaug.hip -- RandAugment on decoded uint8 frames, one layer (one op slot of the policy) of a whole batch per call
// (datasets/rand_augment.py of the reference, which runs the ops through PIL on a loader worker).  The arithmetic is PIL's,
// bit for bit; include/focus_amd.h states it op by op.
//
// Work split of the apply kernel: blockIdx.y is the frame, so the descriptor and the op are block-uniform; a thread owns PIX = 4
// consecutive pixels of one row, 12 bytes, loaded and stored as one three-dword access at any byte address when the run is
// whole, byte by byte at a row's end (W need not be a multiple of 4).  Neighbour reads (the 3x3 filter,
// the affine gathers) are bytes out of the vector cache.  Table ops build their 3 x 256 table in LDS at the start of every
// workgroup: closed forms directly, AutoContrast / Equalize from the frame's histogram in the workspace (768 words, an LDS
// scan), so no launch sits between the stats and the apply launch and nothing returns to the host.
//
// Stats kernel: a workgroup histograms 8192 pixels into one LDS histogram per wave (a wave's lanes hit the same bins on smooth
// content; four copies keep the waves off each other), sums L per lane, and merges its non-zero bins into the frame's slot
// with vector atomics.  Integer sums: the same words whatever the order.
//
// Rounding contract: contraction is off for the whole file.  An fma would skip the rounding of the product in the blends, the
// table arithmetic and the fp64 filters, and PIL's C code rounds each operation.
#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int PIX = 4;
constexpr int STAT_PIX = 8192;
constexpr int STAT_WORDS = FOCUS_RANDAUG_STAT_WORDS;
constexpr int MAX_DIM = 32768;

__device__ __forceinline__ int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ uint8_t clip8f(float t) { return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (uint8_t)t; }

// Image.blend(degenerate, image, factor): degenerate + factor * (image - degenerate), two roundings, clamp, truncate.
// Plain operators under this file's contract(off), as in mixup.hip: HIP's __fmul_rn / __fadd_rn are header inlines (x * y,
// x + y) compiled under the default contraction, and the pair fuses into one fma once inlined here.
__device__ __forceinline__ uint8_t blend(int d, int v, float f) {
    const float prod = f * (float)(v - d);
    return clip8f((float)d + prod);
}

__device__ __forceinline__ bool stats_slot_ok(const focus_randaug_item& it, int64_t ws_words) {
    return it.stats_off >= 0 && (it.stats_off & 1) == 0 && it.stats_off + STAT_WORDS <= ws_words;
}

__global__ __launch_bounds__(THREADS) void randaug_stats_kernel(const focus_randaug_item* __restrict__ items,
                                                                uint32_t* __restrict__ ws, int64_t ws_words, int max_h,
                                                                int max_w) {
    const focus_randaug_item it = items[blockIdx.y];
    if (!stats_slot_ok(it, ws_words) || it.H <= 0 || it.W <= 0 || it.H > max_h || it.W > max_w) return;
    if (it.op != FOCUS_RA_AUTOCONTRAST && it.op != FOCUS_RA_EQUALIZE && it.op != FOCUS_RA_CONTRAST) return;
    const int npix = it.H * it.W;
    const int p0 = blockIdx.x * STAT_PIX;
    if (p0 >= npix) return;
    __shared__ uint32_t h[4][768];
    __shared__ unsigned long long lsum;
    for (int i = threadIdx.x; i < 4 * 768; i += THREADS) (&h[0][0])[i] = 0;
    if (threadIdx.x == 0) lsum = 0;
    __syncthreads();
    uint32_t* hw = h[threadIdx.x >> 6];
    const int p1 = min(p0 + STAT_PIX, npix);
    uint32_t mine = 0;
    for (int p = p0 + threadIdx.x; p < p1; p += THREADS) {
        const int y = p / it.W, x = p - y * it.W;
        const uint8_t* s = it.src + (int64_t)y * it.src_stride + 3 * x;
        const int r = s[0], g = s[1], b = s[2];
        atomicAdd(&hw[r], 1u);
        atomicAdd(&hw[256 + g], 1u);
        atomicAdd(&hw[512 + b], 1u);
        mine += (uint32_t)lum(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&lsum, (unsigned long long)mine);
    __syncthreads();
    uint32_t* out = ws + it.stats_off;
    for (int i = threadIdx.x; i < 768; i += THREADS) {
        const uint32_t v = h[0][i] + h[1][i] + h[2][i] + h[3][i];
        if (v) atomicAdd(&out[i], v);
    }
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + 768), lsum);
}

// 3 x 256 table of a table op; all THREADS threads of the workgroup call it (thread v owns entry v of each channel)
__device__ void build_lut(const focus_randaug_item& it, const uint32_t* __restrict__ st, uint8_t (*lut)[256], int (*scan)[256],
                          int* red) {
    const int v = threadIdx.x;
    const int op = it.op;
    if (op == FOCUS_RA_AUTOCONTRAST || op == FOCUS_RA_EQUALIZE) {
        int hc[3];
        if (v < 9) red[v] = (v < 3) ? 256 : (v < 6) ? -1 : 0;          // lo[3], hi[3], occupied bins[3]
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hc[c] = st ? (int)st[c * 256 + v] : 0;
            scan[c][v] = hc[c];
            if (hc[c]) {
                atomicMin(&red[c], v);
                atomicMax(&red[3 + c], v);
                atomicAdd(&red[6 + c], 1);
            }
        }
        __syncthreads();
        if (op == FOCUS_RA_AUTOCONTRAST) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int lo = red[c], hi = red[3 + c];
                int o = v;
                if (hi > lo) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double offset = -(double)lo * scale;
                    const int ix = (int)((double)v * scale + offset);
                    o = ix < 0 ? 0 : ix > 255 ? 255 : ix;
                }
                lut[c][v] = (uint8_t)o;
            }
            return;
        }
        for (int o = 1; o < 256; o <<= 1) {                              // inclusive scan of the three histograms
            int t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = v >= o ? scan[c][v - o] : 0;
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 3; ++c) scan[c][v] += t[c];
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int hi = red[3 + c];
            int o = v;
            if (red[6 + c] > 1) {
                const int last = scan[c][hi] - (hi > 0 ? scan[c][hi - 1] : 0);
                const int step = (scan[c][255] - last) / 255;
                if (step > 0) o = min(255, (step / 2 + scan[c][v] - hc[c]) / step);
            }
            lut[c][v] = (uint8_t)o;
        }
        return;
    }
    int o = v;
    if (op == FOCUS_RA_INVERT) {
        o = 255 - v;
    } else if (op == FOCUS_RA_POSTERIZE) {
        o = it.iarg >= 8 ? v : it.iarg <= 0 ? 0 : (v & ~((1 << (8 - it.iarg)) - 1));
    } else if (op == FOCUS_RA_SOLARIZE) {
        o = v < it.iarg ? v : 255 - v;
    } else if (op == FOCUS_RA_SOLARIZE_ADD) {
        o = v < 128 ? min(255, max(0, v + it.iarg)) : v;
    } else if (op == FOCUS_RA_BRIGHTNESS) {
        o = blend(0, v, it.farg);
    }
    lut[0][v] = lut[1][v] = lut[2][v] = (uint8_t)o;
}

struct Src {
    const uint8_t* p;
    int64_t stride;
    int H, W;
    __device__ __forceinline__ const uint8_t* row(int y) const { return p + (int64_t)y * stride; }
};
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : v < n ? v : n - 1; }

#define BILINEAR(a, b, d) ((a) + ((b) - (a)) * (d))
__device__ __forceinline__ double bicubic1(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// PIL's bilinear_filter32RGB / bicubic_filter32RGB at the source point (xin, yin), which lies inside the frame
__device__ __forceinline__ void resample_px(const Src& s, double xin, double yin, int bicubic, uint8_t* out) {
    xin -= 0.5;
    yin -= 0.5;
    int x = xin >= 0.0 ? (int)xin : (int)floor(xin);
    int y = yin >= 0.0 ? (int)yin : (int)floor(yin);
    const double dx = xin - x, dy = yin - y;
    if (!bicubic) {
        const int x0 = clampi(x, s.W) * 3, x1 = clampi(x + 1, s.W) * 3;
        const uint8_t* r0 = s.row(clampi(y, s.H));
        const bool has1 = y + 1 >= 0 && y + 1 < s.H;
        const uint8_t* r1 = has1 ? s.row(y + 1) : r0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v1 = BILINEAR((double)r0[x0 + c], (double)r0[x1 + c], dx);
            const double v2 = has1 ? BILINEAR((double)r1[x0 + c], (double)r1[x1 + c], dx) : v1;
            out[c] = (uint8_t)BILINEAR(v1, v2, dy);
        }
        return;
    }
    --x;
    --y;
    const int x0 = clampi(x, s.W) * 3, x1 = clampi(x + 1, s.W) * 3, x2 = clampi(x + 2, s.W) * 3, x3 = clampi(x + 3, s.W) * 3;
    const uint8_t* r[4];
    bool has[4];
    r[0] = s.row(clampi(y, s.H));
    has[0] = true;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        has[k] = y + k >= 0 && y + k < s.H;
        r[k] = has[k] ? s.row(y + k) : r[0];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = (k == 0 || has[k])
                       ? bicubic1((double)r[k][x0 + c], (double)r[k][x1 + c], (double)r[k][x2 + c], (double)r[k][x3 + c], dx)
                       : v[k - 1];
        const double o = bicubic1(v[0], v[1], v[2], v[3], dy);
        out[c] = o <= 0.0 ? 0 : o >= 255.0 ? 255 : (uint8_t)o;
    }
}

__global__ __launch_bounds__(THREADS) void randaug_apply_kernel(const focus_randaug_item* __restrict__ items,
                                                                const uint32_t* __restrict__ ws, int64_t ws_words, int max_h,
                                                                int max_w) {
    __shared__ uint8_t lut[3][256];
    __shared__ int scan[3][256];
    __shared__ int red[12];
    const focus_randaug_item it = items[blockIdx.y];
    if (it.H <= 0 || it.W <= 0 || it.H > max_h || it.W > max_w) return;
    const int runs = (it.W + PIX - 1) / PIX;
    const int total = runs * it.H;
    if ((int)(blockIdx.x * THREADS) >= total) return;                    // block-uniform: before any barrier
    const uint32_t* st = (ws && stats_slot_ok(it, ws_words)) ? ws + it.stats_off : nullptr;
    int op = it.op;
    if (op < 0 || op > FOCUS_RA_TRANSLATE_Y) op = FOCUS_RA_COPY;
    if (!st && (op == FOCUS_RA_AUTOCONTRAST || op == FOCUS_RA_EQUALIZE || op == FOCUS_RA_CONTRAST)) op = FOCUS_RA_COPY;
    const bool table = op >= FOCUS_RA_AUTOCONTRAST && op <= FOCUS_RA_BRIGHTNESS;
    if (table) {
        build_lut(it, st, lut, scan, red);
        __syncthreads();
    }
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const int y = idx / runs, xb = (idx - y * runs) * PIX;
    const int n = min(PIX, it.W - xb);
    const uint8_t* srow = it.src + (int64_t)y * it.src_stride + 3 * xb;
    uint8_t* drow = it.dst + (int64_t)y * it.dst_stride + 3 * xb;

    // 12 bytes at any byte address: the target allows unaligned dword access to global memory, so the compiler keeps these one
    // three-dword access (rows of 3 W bytes start on a dword boundary only every fourth row when W is odd)
    struct __attribute__((packed, aligned(1))) Run12 { uint32_t w[3]; };
    union Run { uint32_t w[3]; uint8_t b[12]; } in, out;
    in.w[0] = in.w[1] = in.w[2] = 0;
    const bool affine = op >= FOCUS_RA_ROTATE;
    if (!affine) {
        if (n == PIX) {
            const Run12 r = *reinterpret_cast<const Run12*>(srow);
            in.w[0] = r.w[0]; in.w[1] = r.w[1]; in.w[2] = r.w[2];
        } else {
            for (int k = 0; k < 3 * n; ++k) in.b[k] = srow[k];
        }
    }
    out = in;
    if (table) {
#pragma unroll
        for (int k = 0; k < 3 * PIX; ++k) out.b[k] = lut[k % 3][in.b[k]];
    } else if (op == FOCUS_RA_COLOR) {
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int L = lum(in.b[3 * j], in.b[3 * j + 1], in.b[3 * j + 2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) out.b[3 * j + c] = blend(L, in.b[3 * j + c], it.farg);
        }
    } else if (op == FOCUS_RA_CONTRAST) {
        const unsigned long long sum = *reinterpret_cast<const unsigned long long*>(st + 768);
        const int grey = (int)((double)sum / (double)((int64_t)it.H * it.W) + 0.5);
#pragma unroll
        for (int k = 0; k < 3 * PIX; ++k) out.b[k] = blend(grey, in.b[k], it.farg);
    } else if (op == FOCUS_RA_SHARPNESS) {
        constexpr float K1 = 1.0f / 13.0f, K5 = 5.0f / 13.0f;
        const bool yin = y > 0 && y < it.H - 1;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int x = xb + j;
            if (j >= n || !yin || x == 0 || x == it.W - 1) continue;               // border pixels: degenerate == image, out = in
            const uint8_t* up = srow + 3 * j - it.src_stride;
            const uint8_t* mid = srow + 3 * j;
            const uint8_t* dn = srow + 3 * j + it.src_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ss = 0.5f;
                ss += (float)dn[c - 3] * K1 + (float)dn[c] * K1 + (float)dn[c + 3] * K1;
                ss += (float)mid[c - 3] * K1 + (float)mid[c] * K5 + (float)mid[c + 3] * K1;
                ss += (float)up[c - 3] * K1 + (float)up[c] * K1 + (float)up[c + 3] * K1;
                out.b[3 * j + c] = blend(clip8f(ss), in.b[3 * j + c], it.farg);
            }
        }
    } else if (affine) {
        const Src s{it.src, it.src_stride, it.H, it.W};
        const double yc = (double)y + 0.5;
        const int bicubic = it.resample == FOCUS_RA_BICUBIC;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (j >= n) continue;
            const double xc = (double)(xb + j) + 0.5;
            const double xs = it.coef[0] * xc + it.coef[1] * yc + it.coef[2];
            const double ys = it.coef[3] * xc + it.coef[4] * yc + it.coef[5];
            if (xs < 0.0 || xs >= (double)it.W || ys < 0.0 || ys >= (double)it.H || !(xs == xs) || !(ys == ys)) {
                out.b[3 * j] = it.fill[0]; out.b[3 * j + 1] = it.fill[1]; out.b[3 * j + 2] = it.fill[2];
            } else {
                resample_px(s, xs, ys, bicubic, &out.b[3 * j]);
            }
        }
    }
    if (n == PIX) {
        Run12 r;
        r.w[0] = out.w[0]; r.w[1] = out.w[1]; r.w[2] = out.w[2];
        *reinterpret_cast<Run12*>(drow) = r;
    } else {
        for (int k = 0; k < 3 * n; ++k) drow[k] = out.b[k];
    }
}

}  // namespace

extern "C" size_t focus_randaug_workspace_bytes(int n_stats_frames) {
    return n_stats_frames <= 0 ? 0 : (size_t)n_stats_frames * STAT_WORDS * sizeof(uint32_t);
}

extern "C" int focus_randaug_layer(const focus_randaug_item* items, int n_items, int max_h, int max_w, int need_stats,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!items || (need_stats && !workspace)) return FOCUS_ERR_NULL;
    if (n_items <= 0) return FOCUS_OK;
    if (max_h < 1 || max_w < 1 || max_h > MAX_DIM || max_w > MAX_DIM || n_items > 65535) return FOCUS_ERR_SHAPE;
    if (workspace && !focus_aligned(workspace, 8)) return FOCUS_ERR_ALIGN;
    if (need_stats && workspace_bytes < focus_randaug_workspace_bytes(1)) return FOCUS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ws_words = workspace ? (int64_t)(workspace_bytes / sizeof(uint32_t)) : 0;
    if (need_stats) {
        const dim3 grid((unsigned)cdiv64((int64_t)max_h * max_w, STAT_PIX), (unsigned)n_items);
        randaug_stats_kernel<<<grid, THREADS, 0, s>>>(items, (uint32_t*)workspace, ws_words, max_h, max_w);
        FOCUS_CHECK_LAUNCH();
    }
    const int64_t work = (int64_t)((max_w + PIX - 1) / PIX) * max_h;      // <= 8192 * 32768: fits an int
    const dim3 grid((unsigned)cdiv64(work, THREADS), (unsigned)n_items);
    randaug_apply_kernel<<<grid, THREADS, 0, s>>>(items, (const uint32_t*)workspace, ws_words, max_h, max_w);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
