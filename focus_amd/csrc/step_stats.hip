// step_stats.hip -- what the training, validation and test loops do with the predictions, on the device and without a host
// round trip.
//
//   focus_topk_stats       one batch of logits (one or two heads, int64 or dense mixup labels) and up to three loss scalars ->
//                          added into a small accumulator that stays on the device: top-k correct counts per head and for
//                          "every head" (the EPIC-Kitchens action), steps, samples, the loss sums in double, and the step of
//                          the first NaN loss (the deferred form of misc.check_nan_losses).
//   focus_view_accumulate  the multi-view ensembling of TestMeter / EPICTestMeter: the clips of a batch are folded into
//                          their videos' rows of an fp32 table in ascending row order.
//
// Counts are integers added with integer atomics, so they are the same in any arrival order.  The loss sums are doubles
// touched by exactly one thread per launch, in launch order: the same bits as the host's sums in step order.  No float
// atomics anywhere.  Contraction is off for the file: the collapsed mixup score rounds once, like the torch add.
#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAXNK = 4;
// int64 table: 0 steps, 1 samples, 2 NaN latched (0 / 1), 3 step of the first NaN, 4 + 4 h + k correct[h][k] (h = 2: every head)
constexpr int ACC_STEPS = 0, ACC_SAMPLES = 1, ACC_NAN = 2, ACC_NAN_STEP = 3, ACC_CORRECT = 4;
// float64 table: 0..2 loss_sum, 3..5 loss_weighted

struct head_t {
    const void* logits;
    const void* labels;
    int64_t ld, ldl;
    int V, bf16;
};
struct ks_t { int k[MAXNK]; };

__device__ __forceinline__ float ldv(const void* p, int64_t i, int bf16) {
    return bf16 ? bf16_to_f32(reinterpret_cast<const bf16_t*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// (x, i) beats (y, j): NaN is greatest, then the larger value, then the lower index.  Two NaNs do not beat each other.
__device__ __forceinline__ bool beats(float x, int i, float y, int j) {
    const bool xn = x != x, yn = y != y;
    if (xn != yn) return xn;
    return x > y || (x == y && i < j);
}
// the same with two NaNs ordered by index, so that the greatest entry of a row is one entry whatever the scan order
__device__ __forceinline__ bool before(float x, int i, float y, int j) {
    const bool xn = x != x, yn = y != y;
    if (xn && yn) return i < j;
    return beats(x, i, y, j);
}

__device__ __forceinline__ void wave_argmax(float& v, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (oi >= 0 && (idx < 0 || before(ov, oi, v, idx))) {
            v = ov;
            idx = oi;
        }
    }
}

// How many entries of the row beat the label's entry; -1 when the row has no label inside [0, V).  One wave per row.
__device__ int row_rank(const head_t& h, int64_t row, int dense, int lane) {
    const int V = h.V;
    const int64_t base = row * h.ld;
    int label, second = -1;
    float x, zero_at_second = 0.f;
    if (!dense) {
        const int64_t l = reinterpret_cast<const int64_t*>(h.labels)[row];
        if (l < 0 || l >= V) return -1;
        label = (int)l;
        x = ldv(h.logits, base + label, h.bf16);
    } else {
        const float* lab = reinterpret_cast<const float*>(h.labels) + row * h.ldl;
        float bv = 0.f;
        int bi = -1;
        for (int j = lane; j < V; j += 64) {
            const float v = lab[j];
            if (bi < 0 || before(v, j, bv, bi)) { bv = v; bi = j; }
        }
        wave_argmax(bv, bi);
        label = bi;
        bv = 0.f;
        bi = -1;
        for (int j = lane; j < V; j += 64) {
            const float v = lab[j];
            if (j != label && (bi < 0 || before(v, j, bv, bi))) { bv = v; bi = j; }
        }
        wave_argmax(bv, bi);
        second = bi;
        // pred[first] += pred[second] of the torch collapse: the fp32 sum, rounded once to the logits' type
        x = ldv(h.logits, base + label, h.bf16) + ldv(h.logits, base + second, h.bf16);
        if (h.bf16) x = bf16_to_f32(f32_to_bf16(x));
    }
    int n = 0;
    for (int j = lane; j < V; j += 64) {
        if (j == label) continue;
        const float v = j == second ? zero_at_second : ldv(h.logits, base + j, h.bf16);
        n += beats(v, j, x, label) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    return n;
}

__global__ __launch_bounds__(THREADS) void topk_stats_kernel(head_t h0, head_t h1, int heads, int B, int dense, int nk, ks_t ks,
                                                             const float* loss0, const float* loss1, const float* loss2,
                                                             unsigned long long* acc_i, double* acc_f) {
    __shared__ int s_cnt[3 * MAXNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3 * MAXNK) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
    if (heads > 0 && row < B) {
        const int r0 = row_rank(h0, row, dense, lane);
        const int r1 = heads > 1 ? row_rank(h1, row, dense, lane) : r0;
        if (lane < nk) {
            const int k = ks.k[lane];
            const bool c0 = r0 >= 0 && r0 < k, c1 = r1 >= 0 && r1 < k;
            if (c0) atomicAdd(&s_cnt[lane], 1);
            if (heads > 1 && c1) atomicAdd(&s_cnt[MAXNK + lane], 1);
            if (c0 && c1) atomicAdd(&s_cnt[2 * MAXNK + lane], 1);
        }
    }
    __syncthreads();
    if (tid < 3 * MAXNK && s_cnt[tid]) atomicAdd(acc_i + ACC_CORRECT + tid, (unsigned long long)s_cnt[tid]);
    if (blockIdx.x == 0 && tid == 0) {
        // the one thread of the launch that touches the scalars
        const unsigned long long steps = acc_i[ACC_STEPS];
        const float* loss[3] = {loss0, loss1, loss2};
        for (int i = 0; i < 3; ++i) {
            if (!loss[i]) continue;
            const double l = (double)*loss[i];
            acc_f[i] = acc_f[i] + l;
            acc_f[3 + i] = acc_f[3 + i] + l * (double)B;
        }
        if (loss0 && *loss0 != *loss0 && acc_i[ACC_NAN] == 0) {
            acc_i[ACC_NAN] = 1;
            acc_i[ACC_NAN_STEP] = steps;
        }
        acc_i[ACC_STEPS] = steps + 1;
        acc_i[ACC_SAMPLES] = acc_i[ACC_SAMPLES] + (unsigned long long)B;
    }
}

// ---- focus_view_accumulate ---------------------------------------------------------------------------------------------
// Workgroup (i, y): row i of the batch, columns [256 y, 256 y + 256).  The row is the owner of its video when no earlier row
// of the batch has the same video; an owner starts from the table's row and folds every row of its video in ascending row
// order, which is the order of the reference's per-clip loop.  Owners have distinct videos, so no two workgroups write one
// table row.  Column chunk 0's first thread walks the labels and the count the same way.
__global__ __launch_bounds__(THREADS) void view_accumulate_kernel(const void* __restrict__ preds, int bf16, int n, int C, int64_t ld,
                                                                  const int64_t* __restrict__ clip_ids,
                                                                  const int64_t* __restrict__ labels, int64_t num_clips,
                                                                  int64_t num_videos, int mode, float* video_preds,
                                                                  int64_t* video_labels, int64_t* clip_count, int* flag) {
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const int64_t total = num_videos * num_clips;
    const int64_t id = clip_ids[i];
    if (id < 0 || id >= total) {
        if (tid == 0 && blockIdx.y == 0) atomicOr(flag, 2);
        return;
    }
    const int64_t vid = id / num_clips;
    int earlier = 0;
    for (int j = tid; j < i; j += THREADS) {
        const int64_t o = clip_ids[j];
        earlier |= (o >= 0 && o < total && o / num_clips == vid) ? 1 : 0;
    }
    if (__syncthreads_or(earlier)) return;
    const int c = blockIdx.y * THREADS + tid;
    if (c < C) {
        float acc = video_preds[vid * C + c];
        for (int j = i; j < n; ++j) {
            const int64_t o = clip_ids[j];
            if (o < 0 || o >= total || o / num_clips != vid) continue;
            const float p = ldv(preds, (int64_t)j * ld + c, bf16);
            if (mode == FOCUS_VIEW_SUM)
                acc = acc + p;
            else
                acc = (p != p || p > acc) ? p : acc;                          // torch.max: a NaN stays
        }
        video_preds[vid * C + c] = acc;
    }
    if (blockIdx.y == 0 && tid == 0) {
        int64_t stored = video_labels[vid], cnt = 0;
        bool conflict = false;
        for (int j = i; j < n; ++j) {
            const int64_t o = clip_ids[j];
            if (o < 0 || o >= total || o / num_clips != vid) continue;
            const int64_t l = labels[j];
            conflict |= stored != 0 && stored != l;
            stored = l;
            ++cnt;
        }
        video_labels[vid] = stored;
        clip_count[vid] = clip_count[vid] + cnt;
        if (conflict) atomicOr(flag, 1);
    }
}

}  // namespace

extern "C" int focus_topk_stats(int heads, int B, const void* logits0, int dtype0, int V0, int64_t ld0, const void* labels0,
                                int64_t ldl0, const void* logits1, int dtype1, int V1, int64_t ld1, const void* labels1,
                                int64_t ldl1, int dense_labels, int nk, int k0, int k1, int k2, int k3, const float* loss0,
                                const float* loss1, const float* loss2, int64_t* acc_i, double* acc_f, void* stream) {
    if (!acc_i || !acc_f) return FOCUS_ERR_NULL;
    if (heads < 0 || heads > 2) return FOCUS_ERR_SHAPE;
    head_t h[2] = {{logits0, labels0, ld0, ldl0, V0, dtype0 == FOCUS_BF16}, {logits1, labels1, ld1, ldl1, V1, dtype1 == FOCUS_BF16}};
    const int dt[2] = {dtype0, dtype1};
    for (int i = 0; i < heads; ++i)
        if (!h[i].logits || !h[i].labels) return FOCUS_ERR_NULL;
    ks_t ks = {{k0, k1, k2, k3}};
    if (heads > 0) {
        if (nk < 1 || nk > MAXNK) return FOCUS_ERR_SHAPE;
        for (int j = 0; j < nk; ++j)
            if (ks.k[j] < 1 || (j && ks.k[j] <= ks.k[j - 1])) return FOCUS_ERR_SHAPE;
        for (int i = 0; i < heads; ++i) {
            if (h[i].V < 1 || (dense_labels && h[i].V < 2) || ks.k[nk - 1] > h[i].V) return FOCUS_ERR_SHAPE;
            if (h[i].ld < h[i].V || (dense_labels && h[i].ldl < h[i].V)) return FOCUS_ERR_SHAPE;
        }
        for (int i = 0; i < heads; ++i)
            if (dt[i] != FOCUS_F32 && dt[i] != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    }
    if (B <= 0) return FOCUS_OK;
    const unsigned blocks = heads > 0 ? (unsigned)cdiv64(B, WAVES) : 1u;
    topk_stats_kernel<<<dim3(blocks), THREADS, 0, (hipStream_t)stream>>>(h[0], h[1], heads, B, dense_labels ? 1 : 0, nk, ks, loss0,
                                                                         loss1, loss2, (unsigned long long*)acc_i, acc_f);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_view_accumulate(const void* preds, int dtype, int n, int C, int64_t ld, const int64_t* clip_ids,
                                     const int64_t* labels, int num_clips, int num_videos, int mode, float* video_preds,
                                     int64_t* video_labels, int64_t* clip_count, int32_t* flag, void* stream) {
    if (!preds || !clip_ids || !labels || !video_preds || !video_labels || !clip_count || !flag) return FOCUS_ERR_NULL;
    if (num_clips < 1 || num_videos < 0 || C < 1 || ld < C) return FOCUS_ERR_SHAPE;
    if (mode != FOCUS_VIEW_SUM && mode != FOCUS_VIEW_MAX) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (n <= 0) return FOCUS_OK;
    const int64_t chunks = cdiv64(C, THREADS);
    if (chunks > 65535) return FOCUS_ERR_SHAPE;
    view_accumulate_kernel<<<dim3((unsigned)n, (unsigned)chunks), THREADS, 0, (hipStream_t)stream>>>(
        preds, dtype == FOCUS_BF16, n, C, ld, clip_ids, labels, num_clips, num_videos, mode, video_preds, video_labels, clip_count,
        flag);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
