// multilabel.hip -- the multi-label route (DATA.MULTI_LABEL): what the loss, the test meter and the epoch-end mAP do, on the
// device.
//
//   focus_bce_rows               nn.BCEWithLogitsLoss / nn.BCELoss over [R,C] rows: the row sums and the gradient in one launch.
//   focus_view_accumulate_dense  focus_view_accumulate with dense fp32 label rows (TestMeter(multi_label=True)).
//   focus_average_precision      get_map: scikit-learn's step-wise average precision per class, by counting instead of sorting,
//                                and the mean over the classes that have a positive.
//
// No float atomics anywhere: every sum has one fixed order, stated where it is made, so the same arguments give the same bits.
// Contraction is off for the file: the formulas in include/focus_amd.h round where they say they round.
#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;

__device__ __forceinline__ float ldv(const void* p, int64_t i, int bf16) {
    return bf16 ? bf16_to_f32(reinterpret_cast<const bf16_t*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// ---- focus_bce_rows ----------------------------------------------------------------------------------------------------
// One workgroup per row.  Thread t adds the elements t, t + 256, ... in ascending order; the 256 partial sums are folded by
// halving (slot s += slot s + h for h = 128, 64, ..., 1).
__global__ __launch_bounds__(THREADS) void bce_rows_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                           int64_t ldy, int C, int mode, float grad_scale,
                                                           float* __restrict__ loss_rows, float* __restrict__ dx, int64_t lddx) {
    __shared__ float red[THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* xr = x + r * ldx;
    const float* yr = y + r * ldy;
    float* dr = dx + r * lddx;
    float acc = 0.f;
    for (int c = tid; c < C; c += THREADS) {
        const float xv = xr[c], yv = yr[c];
        float e, g;
        if (mode == FOCUS_BCE_LOGITS) {
            const float t = expf(-fabsf(xv));                                 // in (0, 1]: never overflows
            e = (fmaxf(xv, 0.f) - xv * yv) + log1pf(t);
            const float s = (xv >= 0.f ? 1.f : t) / (1.f + t);                // sigmoid(x)
            g = s - yv;
        } else {
            const float l1 = fmaxf(logf(xv), -100.f), l0 = fmaxf(log1pf(-xv), -100.f);
            e = -(yv * l1 + (1.f - yv) * l0);
            g = (xv - yv) / fmaxf((1.f - xv) * xv, 1e-12f);
        }
        acc = acc + e;
        dr[c] = grad_scale * g;
    }
    red[tid] = acc;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) loss_rows[r] = red[0];
}

// ---- focus_view_accumulate_dense -----------------------------------------------------------------------------------------
// The geometry and the ownership rule of view_accumulate_kernel (step_stats.hip): workgroup (i, y) is row i of the batch and
// columns [256 y, 256 y + 256); it works only when no earlier row of the batch has the same video, and then folds every row of
// that video in ascending row order, starting from the table's row.  Column chunk 0 also walks the label rows, all C columns of
// them, since the agreement check looks at whole rows.
__global__ __launch_bounds__(THREADS) void view_dense_kernel(const void* __restrict__ preds, int bf16, int n, int C, int64_t ld,
                                                             const int64_t* __restrict__ clip_ids,
                                                             const float* __restrict__ labels, int64_t ldl, int64_t num_clips,
                                                             int64_t num_videos, int mode, float* video_preds, float* video_labels,
                                                             int64_t* clip_count, int* flag) {
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
    if (blockIdx.y != 0) return;
    const float* stored = video_labels + vid * C;                             // the row the next clip is compared with
    int64_t cnt = 0;
    int conflict = 0;
    for (int j = i; j < n; ++j) {                                             // every branch here is the same in all threads
        const int64_t o = clip_ids[j];
        if (o < 0 || o >= total || o / num_clips != vid) continue;
        const float* row = labels + (int64_t)j * ldl;
        int pos = 0, differ = 0;
        for (int k = tid; k < C; k += THREADS) {
            const float a = stored[k], b = row[k];
            pos |= a > 0.f ? 1 : 0;
            differ |= a == b ? 0 : 1;                                         // torch.equal: a NaN equals nothing
        }
        pos = __syncthreads_or(pos);
        differ = __syncthreads_or(differ);
        conflict |= pos & differ;
        stored = row;
        ++cnt;
    }
    for (int k = tid; k < C; k += THREADS) video_labels[vid * C + k] = stored[k];
    if (tid == 0) {
        clip_count[vid] = clip_count[vid] + cnt;
        if (conflict) atomicOr(flag, 1);
    }
}

// ---- focus_average_precision ---------------------------------------------------------------------------------------------
// ap_count_kernel, workgroup (t, c): thread k holds row i = 256 t + k of class c in registers.  The whole column of the class
// is streamed through LDS in tiles of 256 (score, label) pairs; a thread whose row is a positive counts
//     CNT_i = #{j : s_j >= s_i}      TP_i = #{j : s_j >= s_i and y_j == 1}
// (a wave without a positive only helps to load).  Every LDS read of the counting loop is one address for the whole wave: a
// broadcast, no bank conflict.  The quotient TP_i / CNT_i is taken in double (0 for a row that is no positive) and the 256
// quotients are folded by halving in LDS: slot s += slot s + h for h = 128, ..., 1.  The workgroup writes that partial sum,
// its number of non-zero labels and its flag bits to the workspace.  ap_finish_kernel: thread per class adds the partial
// sums in ascending tile order and divides by the number of positives; after a barrier thread 0 takes the mean over the kept
// classes in ascending class order.
constexpr int AP_BAD_LABEL = 1, AP_BAD_SCORE = 2, AP_NO_CLASS = 4;

__global__ __launch_bounds__(THREADS) void ap_count_kernel(const float* __restrict__ scores, int64_t lds_,
                                                           const float* __restrict__ labels, int64_t ldl, int N, int tiles,
                                                           double* __restrict__ qpart, int* __restrict__ npart,
                                                           int* __restrict__ fpart) {
    __shared__ __attribute__((aligned(16))) float s_s[THREADS];
    __shared__ __attribute__((aligned(16))) int s_y[THREADS];
    __shared__ double s_q[THREADS];
    __shared__ int s_n, s_f;
    const int tid = threadIdx.x;
    const int t = blockIdx.x, c = blockIdx.y;
    const int64_t i = (int64_t)t * THREADS + tid;
    if (tid == 0) { s_n = 0; s_f = 0; }
    float si = 0.f;
    int pos = 0, nz = 0, bad = 0;
    if (i < N) {
        si = scores[i * lds_ + c];
        const float yi = labels[i * ldl + c];
        pos = yi == 1.f;
        nz = !(yi == 0.f);
        bad = (nz && !pos ? AP_BAD_LABEL : 0) | (fabsf(si) <= 3.402823466e38f ? 0 : AP_BAD_SCORE);      // NaN fails the <=
    }
    const bool wave_counts = __any(pos);
    int cnt = 0, tp = 0;
    for (int64_t base = 0; base < N; base += THREADS) {
        const int64_t j = base + tid;
        __syncthreads();                                                      // the previous tile has been read
        if (j < N) {
            s_s[tid] = scores[j * lds_ + c];
            s_y[tid] = labels[j * ldl + c] == 1.f ? 1 : 0;
        }
        __syncthreads();
        if (!wave_counts) continue;
        const int lim = (int)(N - base < THREADS ? N - base : THREADS);
        int k = 0;
        for (; k + 4 <= lim; k += 4) {
            const float4 s4 = *reinterpret_cast<const float4*>(&s_s[k]);
            const int4 y4 = *reinterpret_cast<const int4*>(&s_y[k]);
            const int g0 = s4.x >= si, g1 = s4.y >= si, g2 = s4.z >= si, g3 = s4.w >= si;
            cnt += g0 + g1 + g2 + g3;
            tp += (g0 & y4.x) + (g1 & y4.y) + (g2 & y4.z) + (g3 & y4.w);
        }
        for (; k < lim; ++k) {
            const int g = s_s[k] >= si;
            cnt += g;
            tp += g & s_y[k];
        }
    }
    // a positive with a finite score counts itself, so cnt >= 1 there; a NaN score counts nothing and is flagged
    s_q[tid] = (pos && cnt > 0) ? (double)tp / (double)cnt : 0.0;
    if (nz) atomicAdd(&s_n, 1);
    if (bad) atomicOr(&s_f, bad);
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) s_q[tid] = s_q[tid] + s_q[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = (int64_t)c * tiles + t;
        qpart[o] = s_q[0];
        npart[o] = s_n;
        fpart[o] = s_f;
    }
}

__global__ __launch_bounds__(THREADS) void ap_finish_kernel(int C, int tiles, const double* __restrict__ qpart,
                                                            const int* __restrict__ npart, const int* __restrict__ fpart,
                                                            int64_t* npos, double* ap, double* summary, int* flag) {
    __shared__ int s_f;
    const int tid = threadIdx.x;
    if (tid == 0) s_f = 0;
    __syncthreads();
    for (int c = tid; c < C; c += THREADS) {
        double q = 0.0;
        int64_t np = 0;
        int f = 0;
        for (int t = 0; t < tiles; ++t) {
            const int64_t o = (int64_t)c * tiles + t;
            q = q + qpart[o];
            np += npart[o];
            f |= fpart[o];
        }
        npos[c] = np;
        ap[c] = np > 0 ? q / (double)np : 0.0;
        if (np > 0 && f) atomicOr(&s_f, f);
    }
    __syncthreads();                                                          // ap and npos of this workgroup are visible to it
    if (tid == 0) {
        double sum = 0.0;
        int64_t kept = 0;
        for (int c = 0; c < C; ++c)
            if (npos[c] > 0) {
                sum = sum + ap[c];
                ++kept;
            }
        summary[0] = kept > 0 ? sum / (double)kept : 0.0;
        summary[1] = (double)kept;
        flag[0] = s_f | (kept > 0 ? 0 : AP_NO_CLASS);
    }
}

}  // namespace

extern "C" int focus_bce_rows(const float* x, int64_t ldx, const float* y, int64_t ldy, int R, int C, int mode, float grad_scale,
                              float* loss_rows, float* dx, int64_t lddx, void* stream) {
    if (!x || !y || !loss_rows || !dx) return FOCUS_ERR_NULL;
    if (R < 0 || C < 1 || ldx < C || ldy < C || lddx < C) return FOCUS_ERR_SHAPE;
    if (mode != FOCUS_BCE_LOGITS && mode != FOCUS_BCE_PROBS) return FOCUS_ERR_SHAPE;
    if (R == 0) return FOCUS_OK;
    bce_rows_kernel<<<dim3((unsigned)R), THREADS, 0, (hipStream_t)stream>>>(x, ldx, y, ldy, C, mode, grad_scale, loss_rows, dx, lddx);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_view_accumulate_dense(const void* preds, int dtype, int n, int C, int64_t ld, const int64_t* clip_ids,
                                           const float* labels, int64_t ldl, int num_clips, int num_videos, int mode,
                                           float* video_preds, float* video_labels, int64_t* clip_count, int32_t* flag,
                                           void* stream) {
    if (!preds || !clip_ids || !labels || !video_preds || !video_labels || !clip_count || !flag) return FOCUS_ERR_NULL;
    if (num_clips < 1 || num_videos < 0 || C < 1 || ld < C || ldl < C) return FOCUS_ERR_SHAPE;
    if (mode != FOCUS_VIEW_SUM && mode != FOCUS_VIEW_MAX) return FOCUS_ERR_SHAPE;
    const int64_t chunks = cdiv64(C, THREADS);
    if (chunks > 65535) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (n <= 0) return FOCUS_OK;
    view_dense_kernel<<<dim3((unsigned)n, (unsigned)chunks), THREADS, 0, (hipStream_t)stream>>>(
        preds, dtype == FOCUS_BF16, n, C, ld, clip_ids, labels, ldl, num_clips, num_videos, mode, video_preds, video_labels,
        clip_count, flag);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" size_t focus_average_precision_workspace_bytes(int N, int C) {
    if (N < 1 || C < 1) return 0;
    return (size_t)cdiv64(N, THREADS) * (size_t)C * 16;
}

extern "C" int focus_average_precision(const float* scores, int64_t lds, const float* labels, int64_t ldl, int N, int C,
                                       int64_t* npos, double* ap, double* summary, int32_t* flag, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!scores || !labels || !npos || !ap || !summary || !flag) return FOCUS_ERR_NULL;
    if (N < 0 || C < 1 || C > 65535 || lds < C || ldl < C) return FOCUS_ERR_SHAPE;
    const int64_t tiles = cdiv64(N, THREADS);
    if (tiles * C >= (1 << 23)) return FOCUS_ERR_SHAPE;                       // 2^31 threads in the counting launch
    if (N == 0) return FOCUS_OK;                                              // nothing is written: the caller's zeros stand
    if (!workspace) return FOCUS_ERR_NULL;
    if (!focus_aligned(workspace, 8)) return FOCUS_ERR_ALIGN;
    if (workspace_bytes < focus_average_precision_workspace_bytes(N, C)) return FOCUS_ERR_WORKSPACE;
    double* qpart = reinterpret_cast<double*>(workspace);
    int* npart = reinterpret_cast<int*>(qpart + tiles * C);
    int* fpart = npart + tiles * C;
    ap_count_kernel<<<dim3((unsigned)tiles, (unsigned)C), THREADS, 0, (hipStream_t)stream>>>(scores, lds, labels, ldl, N, (int)tiles,
                                                                                             qpart, npart, fpart);
    FOCUS_CHECK_LAUNCH();
    ap_finish_kernel<<<dim3(1), THREADS, 0, (hipStream_t)stream>>>(C, (int)tiles, qpart, npart, fpart, npos, ap, summary, flag);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
