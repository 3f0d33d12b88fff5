// slot_segments.hip -- the hand-off from STEVE's slot attention to ORViT's boxes and to the FG-ARI evaluation, on the
// device and at the slot grid's resolution.
//
//   focus_slot_segments    attns [B,T,N,K] (the slot update's own layout, K innermost) -> the arg-max slot of every cell
//                          (uint8 [B,T,N]) and per (frame, slot) the cell count and the extent (int32 [B,T,K,5]).
//   focus_slot_boxes       the extents -> orvit_bboxes [B,T,O,4] of the O largest slots of each clip, one launch.
//   focus_seg_contingency  segment map (slot grid) x truth masks (full resolution) -> the FG-ARI contingency tables.
//
// Everything produced is an integer, or an fp32 value with one rounding per step of the host chain it restates
// (datasets/utils.boxes_to_orvit_format), so the results are compared bit for bit.  Contraction is off for the file: the
// box arithmetic must round after every operation like numpy / ATen do.
#include <limits.h>

#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAXK = 32;

// ---- focus_slot_segments ------------------------------------------------------------------------------------------------
// Workgroup (frame f, part p of P) owns the cells [p cells_per_wg, (p+1) cells_per_wg) of the frame and walks them 256 at
// a time.  The 256 K scores of a pass are one contiguous byte range of attn: it is copied to LDS as it lies in memory (16-byte
// pieces where the range is aligned, single elements at its two ends; the LDS copy starts at the same offset mod 16 as the
// global range, so both sides of every 16-byte piece are aligned whatever K is), then every thread scans the K scores of its
// cell from LDS.  Lane l starts its scan at slot l % K: with K even the rows of a wave would otherwise sit on a few banks.
// Stats: per wave, lane k reads the extents of slot k off that slot's ballot mask (below), LDS integer atomics per
// workgroup, then either a plain store (P == 1) or global integer atomics into stats that
// stats_init_kernel has set to the empty value.  Integer min / max / add: the result is the same in any arrival order.
__global__ __launch_bounds__(THREADS) void stats_init_kernel(int* __restrict__ stats, int64_t rows, int He, int We) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= rows) return;
    int* s = stats + r * 5;
    s[0] = 0; s[1] = We; s[2] = He; s[3] = -1; s[4] = -1;
}

template <typename T> __device__ __forceinline__ float score(T v);
template <> __device__ __forceinline__ float score<float>(float v) { return v; }
template <> __device__ __forceinline__ float score<bf16_t>(bf16_t v) { return bf16_to_f32(v); }

template <typename T>
__global__ __launch_bounds__(THREADS) void slot_segments_kernel(const T* __restrict__ attn, uint8_t* __restrict__ seg,
                                                                int* __restrict__ stats, int N, int He, int We, int K, int P,
                                                                int cells_per_wg) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[THREADS * MAXK * sizeof(T) + 16];
    __shared__ int s_st[MAXK * 5];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t frame = blockIdx.x / P;
    const int part = blockIdx.x - (int)(frame * P);
    const int c_begin = part * cells_per_wg, c_end = min(N, c_begin + cells_per_wg);
    if (tid < K) {
        s_st[tid * 5 + 0] = 0; s_st[tid * 5 + 1] = We; s_st[tid * 5 + 2] = He; s_st[tid * 5 + 3] = -1; s_st[tid * 5 + 4] = -1;
    }
    __syncthreads();
    const T* fbase = attn + frame * N * K;
    for (int c0 = c_begin; c0 < c_end; c0 += THREADS) {
        const int cnt = min(THREADS, c_end - c0);
        const unsigned char* g = reinterpret_cast<const unsigned char*>(fbase + (int64_t)c0 * K);
        const int len = cnt * K * (int)sizeof(T);
        const int off = (int)(reinterpret_cast<uintptr_t>(g) & 15);
        const int head = off ? min(16 - off, len) : 0;                   // bytes in front of the first aligned piece
        const int nvec = (len - head) >> 4;
        const int tail = head + (nvec << 4);                              // bytes [tail, len) behind the last one
        unsigned char* l = raw + off;                                     // l[i] holds g[i]
        for (int v = tid; v < nvec; v += THREADS)
            *reinterpret_cast<uint4*>(l + head + (v << 4)) = *reinterpret_cast<const uint4*>(g + head + (v << 4));
        for (int e = tid; e < head / (int)sizeof(T); e += THREADS)
            reinterpret_cast<T*>(l)[e] = reinterpret_cast<const T*>(g)[e];
        for (int e = tid; e < (len - tail) / (int)sizeof(T); e += THREADS)
            reinterpret_cast<T*>(l + tail)[e] = reinterpret_cast<const T*>(g + tail)[e];
        __syncthreads();
        const bool valid = tid < cnt;
        const int n = c0 + tid;
        int bk = 0;
        if (valid) {
            const T* row = reinterpret_cast<const T*>(l) + tid * K;
            int k = tid % K;
            bk = k;
            float best = score<T>(row[k]);
            for (int j = 1; j < K; ++j) {
                k = k + 1 == K ? 0 : k + 1;
                const float v = score<T>(row[k]);
                if (v > best || (v == best && k < bk)) {                   // lowest index among equal maxima
                    best = v;
                    bk = k;
                }
            }
            seg[frame * N + n] = (uint8_t)bk;
        }
        // Stats of the wave's 64 consecutive cells [nw, nw + 64) from ballot masks alone.  Lane k takes the mask of slot k
        // (K <= 32 ballots), so the slots present are worked out side by side.  Lanes ascend with the cell: the first / last
        // set lane of the mask give ymin / ymax, and inside one grid row x ascends with the lane too, so the first / last set
        // lane of the mask cut to a row give that row's xmin / xmax.  No value crosses lanes.
        const int nw = c0 + (tid & ~63);
        unsigned long long m = 0;
        for (int k = 0; k < K; ++k) {
            const unsigned long long mk = __ballot(valid && bk == k);
            if (lane == k) m = mk;
        }
        if (m) {
            const int ymn = (nw + __ffsll(m) - 1) / We, ymx = (nw + 63 - __clzll(m)) / We;
            int xmn = INT_MAX, xmx = -1;
            for (int row = ymn; row <= ymx; ++row) {
                const int lo = max(row * We, nw) - nw, hi = min(row * We + We, nw + 64) - nw;        // the row's lanes [lo, hi)
                const unsigned long long rm = m & ((hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo);
                if (rm) {
                    const int x0 = nw - row * We;                           // x of lane l in this row: x0 + l
                    xmn = min(xmn, x0 + __ffsll(rm) - 1);
                    xmx = max(xmx, x0 + 63 - __clzll(rm));
                }
            }
            atomicAdd(&s_st[lane * 5 + 0], __popcll(m));
            atomicMin(&s_st[lane * 5 + 1], xmn);
            atomicMin(&s_st[lane * 5 + 2], ymn);
            atomicMax(&s_st[lane * 5 + 3], xmx);
            atomicMax(&s_st[lane * 5 + 4], ymx);
        }
        __syncthreads();                                                   // raw is refilled by the next pass
    }
    if (tid < K) {
        int* out = stats + (frame * K + tid) * 5;
        const int* s = s_st + tid * 5;
        if (P == 1) {
            out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = s[3]; out[4] = s[4];
        } else if (s[0] > 0) {
            atomicAdd(out + 0, s[0]);
            atomicMin(out + 1, s[1]);
            atomicMin(out + 2, s[2]);
            atomicMax(out + 3, s[3]);
            atomicMax(out + 4, s[4]);
        }
    }
}

// ---- focus_slot_boxes -----------------------------------------------------------------------------------------------------
// One workgroup per clip: areas by LDS integer adds, the selection by the K threads of the first wave (rank = how many
// candidates come before me in (area descending, index ascending)), then one thread per (frame, object) row.
__global__ __launch_bounds__(THREADS) void slot_boxes_kernel(const int* __restrict__ stats, int T, int K, int H, int W, int sx,
                                                             int sy, int O, int drop_largest, float* __restrict__ boxes,
                                                             int* __restrict__ slot_ids) {
    __shared__ int area[MAXK], kept[MAXK], slot_of[MAXK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int* st = stats + b * T * K * 5;
    if (tid < MAXK) { area[tid] = 0; kept[tid] = 0; }
    __syncthreads();
    for (int i = tid; i < T * K; i += THREADS) {
        const int c = st[(int64_t)i * 5];
        if (c) atomicAdd(&area[i % K], c);
    }
    __syncthreads();
    if (tid < K) {
        int bg = -1;
        if (drop_largest) {
            bg = 0;
            for (int j = 1; j < K; ++j) bg = area[j] > area[bg] ? j : bg;       // ties: the lowest index
        }
        int rank = 0;
        for (int j = 0; j < K; ++j)
            rank += (j != bg && j != tid && area[j] > 0 && (area[j] > area[tid] || (area[j] == area[tid] && j < tid))) ? 1 : 0;
        kept[tid] = tid != bg && area[tid] > 0 && rank < O;
    }
    __syncthreads();
    if (tid < K && kept[tid]) {
        int o = 0;
        for (int j = 0; j < tid; ++j) o += kept[j];
        slot_of[o] = tid;                                                    // ascending slot index
    }
    int nkept = 0;
    for (int j = 0; j < K; ++j) nkept += kept[j];
    __syncthreads();
    for (int o = tid; o < O; o += THREADS) slot_ids[b * O + o] = o < nkept ? slot_of[o] : -1;
    const float fw = (float)W, fh = (float)H;
    for (int64_t i = tid; i < (int64_t)T * O; i += THREADS) {
        const int t = (int)(i / O), o = (int)(i - (int64_t)t * O);
        float cx = 0.f, cy = 0.f, w = 0.f, h = 0.f;
        if (o < nkept) {
            const int* s = st + ((int64_t)t * K + slot_of[o]) * 5;
            if (s[0] > 0) {
                // the pixel box of the nearest-upsampled mask, then boxes_to_orvit_format step by step
                float x0 = (float)(s[1] * sx) / fw, y0 = (float)(s[2] * sy) / fh;
                float x1 = (float)(s[3] * sx + sx - 1) / fw, y1 = (float)(s[4] * sy + sy - 1) / fh;
                x0 = fminf(fmaxf(x0, 0.f), 1.f); y0 = fminf(fmaxf(y0, 0.f), 1.f);
                x1 = fminf(fmaxf(x1, 0.f), 1.f); y1 = fminf(fmaxf(y1, 0.f), 1.f);
                w = x1 - x0;
                h = y1 - y0;
                if (w <= 0.05f || h <= 0.05f) {
                    w = 0.f;
                    h = 0.f;
                } else {
                    cx = (x0 + x1) / 2.f;
                    cy = (y0 + y1) / 2.f;
                }
            }
        }
        float* out = boxes + (b * T * O + i) * 4;
        out[0] = cx; out[1] = cy; out[2] = w; out[3] = h;
    }
}

// ---- focus_seg_contingency ------------------------------------------------------------------------------------------------
// A unit is V consecutive pixels of one row of one truth plane (one vector load; W % V == 0, so a unit never leaves its row).
// The units of one (clip, segment) -- T planes -- are split over `nsplit` workgroups; a lane walks its units, counts runs of
// equal slot in registers and adds a finished run to its WAVE's histogram in LDS.  The workgroup sums its waves and adds
// each non-zero bin to the table with one integer atomic.  The table is zeroed on the stream before the launch.
template <typename T, int V> struct truth_vec;
template <> struct truth_vec<uint8_t, 16> {
    static __device__ __forceinline__ uint32_t nz(const uint8_t* p) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        if (!(u.x | u.y | u.z | u.w)) return 0;                              // most units of a one-hot truth
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) m |= ((w[i >> 2] >> ((i & 3) * 8)) & 0xffu) ? (1u << i) : 0u;
        return m;
    }
};
template <> struct truth_vec<uint8_t, 4> {
    static __device__ __forceinline__ uint32_t nz(const uint8_t* p) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= ((u >> (i * 8)) & 0xffu) ? (1u << i) : 0u;
        return m;
    }
};
template <> struct truth_vec<uint8_t, 1> {
    static __device__ __forceinline__ uint32_t nz(const uint8_t* p) { return *p ? 1u : 0u; }
};
template <> struct truth_vec<float, 4> {
    static __device__ __forceinline__ uint32_t nz(const float* p) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        return (v.x != 0.f ? 1u : 0u) | (v.y != 0.f ? 2u : 0u) | (v.z != 0.f ? 4u : 0u) | (v.w != 0.f ? 8u : 0u);
    }
};
template <> struct truth_vec<float, 1> {
    static __device__ __forceinline__ uint32_t nz(const float* p) { return *p != 0.f ? 1u : 0u; }
};

template <typename T, int V>
__global__ __launch_bounds__(THREADS) void seg_contingency_kernel(const uint8_t* __restrict__ seg, const T* __restrict__ truth,
                                                                  int* __restrict__ table, int Tn, int S, int first, int Sp,
                                                                  int HW, int W, int N, int We, int sx, int sy, int K,
                                                                  int nsplit, int units, int units_per_wg) {
    __shared__ int hist[WAVES][MAXK];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int split = blockIdx.x % nsplit;
    const int bs = blockIdx.x / nsplit;
    const int sp = bs % Sp;
    const int64_t b = bs / Sp;
    if (tid < WAVES * MAXK) hist[tid / MAXK][tid % MAXK] = 0;
    __syncthreads();
    // units < 2^31 (T H W < 2^31), so a unit index plus one stride of the loop fits 32 unsigned bits: no 64-bit division
    const uint32_t u0 = (uint32_t)split * (uint32_t)units_per_wg;
    const uint32_t u1 = min((uint32_t)units, u0 + (uint32_t)units_per_wg);
    const uint32_t cpp = (uint32_t)(HW / V);                                 // units per plane
    int cur_k = -1, cur_n = 0;
    int t = (int)((u0 + tid) / cpp);                                         // plane and unit in the plane, kept by steps
    uint32_t c = (u0 + tid) - (uint32_t)t * cpp;
    for (uint32_t u = u0 + tid; u < u1; u += THREADS, c += THREADS) {
        while (c >= cpp) {
            c -= cpp;
            ++t;
        }
        const int p = (int)c * V;
        const uint32_t nz = truth_vec<T, V>::nz(truth + ((b * Tn + t) * S + sp + first) * HW + p);
        if (!nz) continue;                                                    // most units of a one-hot truth are empty
        const int y = p / W, x = p - y * W;
        const uint8_t* srow = seg + (b * Tn + t) * N + (int64_t)(y / sy) * We;
        // the slot of every pixel of the unit first: V independent byte loads (the frame's map is a few KB, cache hits), one
        // wait; fetched one by one inside the loop below they would be V dependent round trips
        int cx = x / sx, r = x - cx * sx;
        uint8_t ks[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            ks[j] = srow[cx];
            if (++r == sx) {
                r = 0;
                ++cx;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (!((nz >> j) & 1u)) continue;
            if (ks[j] == cur_k) {
                ++cur_n;
            } else {
                if (cur_n && cur_k < K) atomicAdd(&hist[wave][cur_k], cur_n);
                cur_k = ks[j];
                cur_n = 1;
            }
        }
    }
    if (cur_n && cur_k < K) atomicAdd(&hist[wave][cur_k], cur_n);
    __syncthreads();
    if (tid < K) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) v += hist[w][tid];
        if (v) atomicAdd(table + (b * Sp + sp) * K + tid, v);
    }
}

template <typename T, int V>
void launch_contingency(const uint8_t* seg, const void* truth, int* table, int B, int Tn, int S, int first, int H, int W, int He,
                        int We, int K, hipStream_t s) {
    const int Sp = S - first, HW = H * W;
    const int units = (int)((int64_t)Tn * HW / V);
    int64_t nsplit = 2048 / ((int64_t)B * Sp);
    const int64_t most = cdiv64(units, THREADS);
    nsplit = nsplit < 1 ? 1 : nsplit;
    nsplit = nsplit > most ? most : nsplit;
    const int upw = (int)cdiv64(units, nsplit);
    nsplit = cdiv64(units, upw);
    seg_contingency_kernel<T, V><<<dim3((unsigned)((int64_t)B * Sp * nsplit)), THREADS, 0, s>>>(
        seg, (const T*)truth, table, Tn, S, first, Sp, HW, W, He * We, We, W / We, H / He, K, (int)nsplit, units, upw);
}

}  // namespace

extern "C" int focus_slot_segments(const void* attn, int dtype, int B, int T, int He, int We, int K, uint8_t* seg, int32_t* stats,
                                   void* stream) {
    if (!attn || !seg || !stats) return FOCUS_ERR_NULL;
    if (B < 0 || T < 0 || K < 1 || K > MAXK || He < 1 || We < 1) return FOCUS_ERR_SHAPE;
    if ((int64_t)He * We * K > INT_MAX) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (!focus_aligned(attn, focus_esize(dtype)) || !focus_aligned(stats, 4)) return FOCUS_ERR_ALIGN;
    const int64_t frames = (int64_t)B * T;
    if (frames == 0) return FOCUS_OK;
    const int N = He * We;
    // parts per frame: every part at least one pass of 256 cells, and about 2048 workgroups at the most
    int64_t P = cdiv64(N, THREADS);
    const int64_t room = 2048 / frames;
    P = P > room ? (room < 1 ? 1 : room) : P;
    const int passes = (int)cdiv64(cdiv64(N, THREADS), P);
    const int cells_per_wg = passes * THREADS;
    P = cdiv64(N, cells_per_wg);
    if (frames * P > INT_MAX) return FOCUS_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (P > 1) {
        stats_init_kernel<<<dim3((unsigned)cdiv64(frames * K, THREADS)), THREADS, 0, s>>>(stats, frames * K, He, We);
        FOCUS_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)(frames * P));
    if (dtype == FOCUS_BF16)
        slot_segments_kernel<bf16_t><<<grid, THREADS, 0, s>>>((const bf16_t*)attn, seg, stats, N, He, We, K, (int)P, cells_per_wg);
    else
        slot_segments_kernel<float><<<grid, THREADS, 0, s>>>((const float*)attn, seg, stats, N, He, We, K, (int)P, cells_per_wg);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_slot_boxes(const int32_t* stats, int B, int T, int K, int He, int We, int H, int W, int O, int drop_largest,
                                float* boxes, int32_t* slot_ids, void* stream) {
    if (!stats || !boxes || !slot_ids) return FOCUS_ERR_NULL;
    if (B < 0 || T < 0 || O < 0 || K < 1 || K > MAXK || He < 1 || We < 1 || H < 1 || W < 1) return FOCUS_ERR_SHAPE;
    if (H % He != 0 || W % We != 0) return FOCUS_ERR_SHAPE;
    if ((int64_t)T * He * We > INT_MAX || (int64_t)T * K * 5 > INT_MAX || H > (1 << 24) || W > (1 << 24)) return FOCUS_ERR_SHAPE;
    if (!focus_aligned(stats, 4) || !focus_aligned(boxes, 4) || !focus_aligned(slot_ids, 4)) return FOCUS_ERR_ALIGN;
    if (B == 0 || O == 0) return FOCUS_OK;
    slot_boxes_kernel<<<dim3((unsigned)B), THREADS, 0, (hipStream_t)stream>>>(stats, T, K, H, W, W / We, H / He, O, drop_largest,
                                                                             boxes, slot_ids);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_seg_contingency(const uint8_t* seg, const void* truth, int truth_is_f32, int B, int T, int S, int H, int W,
                                     int He, int We, int K, int first_segment, int32_t* table, void* stream) {
    if (!seg || !truth || !table) return FOCUS_ERR_NULL;
    if (B < 0 || T < 0 || S < 1 || H < 1 || W < 1 || He < 1 || We < 1 || K < 1 || K > MAXK) return FOCUS_ERR_SHAPE;
    if (first_segment < 0 || S - first_segment < 1) return FOCUS_ERR_SHAPE;
    if (H % He != 0 || W % We != 0) return FOCUS_ERR_SHAPE;
    if ((int64_t)H * W > INT_MAX || (int64_t)T * H * W > INT_MAX) return FOCUS_ERR_SHAPE;
    const int Sp = S - first_segment;
    if ((int64_t)B * Sp > INT_MAX / MAXK) return FOCUS_ERR_SHAPE;                  // the grid is max(B Sp, 2048) at the most
    if (!focus_aligned(table, 4) || (truth_is_f32 && !focus_aligned(truth, 4))) return FOCUS_ERR_ALIGN;
    if (B == 0) return FOCUS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0, (size_t)B * Sp * K * sizeof(int32_t), s) != hipSuccess) return FOCUS_ERR_LAUNCH;
    if (T == 0) return FOCUS_OK;
    if (truth_is_f32) {
        if (W % 4 == 0 && focus_aligned(truth, 16))
            launch_contingency<float, 4>(seg, truth, table, B, T, S, first_segment, H, W, He, We, K, s);
        else
            launch_contingency<float, 1>(seg, truth, table, B, T, S, first_segment, H, W, He, We, K, s);
    } else {
        if (W % 16 == 0 && focus_aligned(truth, 16))
            launch_contingency<uint8_t, 16>(seg, truth, table, B, T, S, first_segment, H, W, He, We, K, s);
        else if (W % 4 == 0 && focus_aligned(truth, 4))
            launch_contingency<uint8_t, 4>(seg, truth, table, B, T, S, first_segment, H, W, He, We, K, s);
        else
            launch_contingency<uint8_t, 1>(seg, truth, table, B, T, S, first_segment, H, W, He, We, K, s);
    }
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
