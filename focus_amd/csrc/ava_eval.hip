// ava_eval.hip -- the AVA evaluation (PascalBoxes mAP@0.5IOU of slowfast/utils/ava_evaluation) on the device.
//
//   focus_ava_match   the greedy match per (image, class): every detection row of a whitelisted class becomes a false or a
//                     true positive, in the order in which the rows arrived.
//   focus_voc_ap      the VOC average precision per class from that byte table and the scores, by counting instead of sorting,
//                     and the mean over the classes that have ground truth.
//
// No float atomics anywhere (the counters are integers): every double sum has one fixed order, stated where it is made, so
// the same arguments give the same bits.  Contraction is off for the file: the union a + a' - inter must not become an fma of
// the area's product.
#include "focus_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int GT_CAP = 64;                                                    // ground-truth rows per (image, class)
constexpr int MATCH_GT_OVERFLOW = 1, MATCH_BAD_INDEX = 2;
constexpr int VOC_BAD_SCORE = 1, VOC_TP_ABOVE_GT = 2, VOC_GT_ABOVE_TOTAL = 4;

__device__ __forceinline__ float ldv(const void* p, int64_t i, int bf16) {
    return bf16 ? bf16_to_f32(reinterpret_cast<const bf16_t*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// ---- focus_ava_match -----------------------------------------------------------------------------------------------------
// One thread per (group, class); the 256 threads of a workgroup are 256 consecutive classes of one group, so the bytes of a
// row are written side by side.  The thread walks the group's rows in the order of det_rows.  For every valid box it takes the
// IoU with the ground-truth rows of its class in file order, keeps the first maximum, and takes that row when the IoU is at
// least 0.5 and the row is free; the taken rows are the bits of one 64-bit word.
__global__ __launch_bounds__(THREADS) void ava_match_kernel(const float* __restrict__ boxes, int64_t K, int C,
                                                            const int64_t* __restrict__ grp_off,
                                                            const int64_t* __restrict__ det_rows,
                                                            const int64_t* __restrict__ grp_image, int64_t n_images,
                                                            const int64_t* __restrict__ gt_off,
                                                            const int32_t* __restrict__ gt_class,
                                                            const double* __restrict__ gt_boxes,
                                                            const uint8_t* __restrict__ whitelist, uint8_t* __restrict__ out,
                                                            int64_t ldo, unsigned long long* __restrict__ counts,
                                                            int* __restrict__ flag) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    const int64_t g = blockIdx.x;
    if (c >= C || !whitelist[c]) return;
    const int64_t lo = grp_off[g], hi = grp_off[g + 1];
    const int64_t im = grp_image[g];
    if (im >= n_images || lo < 0 || lo > hi || hi > K) {                      // det_rows has K entries
        atomicOr(flag, MATCH_BAD_INDEX);
        return;
    }
    int64_t g0 = 0, g1 = 0;
    if (im >= 0) {
        g0 = gt_off[im];
        g1 = gt_off[im + 1];
    }
    int n_gt = 0;                                                             // ground-truth rows of this class in the image
    for (int64_t t = g0; t < g1; ++t) n_gt += gt_class[t] == c + 1;
    if (n_gt > GT_CAP) {
        atomicOr(flag, MATCH_GT_OVERFLOW);                                    // nothing of this (image, class) is judged
        return;
    }
    unsigned long long taken = 0, n_eval = 0, n_tp = 0;
    for (int64_t k = lo; k < hi; ++k) {
        const int64_t r = det_rows[k];
        if (r < 0 || r >= K) {
            atomicOr(flag, MATCH_BAD_INDEX);
            continue;
        }
        const double x1 = (double)boxes[4 * r], y1 = (double)boxes[4 * r + 1];
        const double x2 = (double)boxes[4 * r + 2], y2 = (double)boxes[4 * r + 3];
        if (!(y1 < y2 && x1 < x2)) continue;                                  // an invalid box is no detection at all
        const double area = (y2 - y1) * (x2 - x1);
        double best = -1.0;
        int best_t = -1, t_cls = 0;
        for (int64_t t = g0; t < g1; ++t) {
            if (gt_class[t] != c + 1) continue;
            const double gx1 = gt_boxes[4 * t], gy1 = gt_boxes[4 * t + 1], gx2 = gt_boxes[4 * t + 2], gy2 = gt_boxes[4 * t + 3];
            const double garea = (gy2 - gy1) * (gx2 - gx1);
            const double ih = fmax(fmin(y2, gy2) - fmax(y1, gy1), 0.0);
            const double iw = fmax(fmin(x2, gx2) - fmax(x1, gx1), 0.0);
            const double inter = ih * iw;
            const double iou = inter / (area + garea - inter);
            if (iou > best) {                                                 // the first maximum wins
                best = iou;
                best_t = t_cls;
            }
            ++t_cls;
        }
        int tp = 0;
        if (best_t >= 0 && best >= 0.5 && !((taken >> best_t) & 1ull)) {
            taken |= 1ull << best_t;
            tp = 1;
        }
        out[r * ldo + c] = tp ? 2 : 1;
        ++n_eval;
        n_tp += tp;
    }
    if (n_eval) atomicAdd(&counts[c], n_eval);
    if (n_tp) atomicAdd(&counts[C + c], n_tp);
}

// ---- focus_voc_ap --------------------------------------------------------------------------------------------------------
// voc_offsets_kernel: one thread clears the flag and lays the classes' precision lists out one behind the other, n_c slots
// each, as long as they fit into total_gt slots.
// voc_rank_kernel, workgroup (t, c): thread k holds row i = 256 t + k of class c.  If the tile has a true positive the whole
// packed column is streamed through LDS in tiles of 256 (key, mark) pairs, and every true positive counts the evaluated rows
// that stand before it in the order of the class -- a higher score, or the same score and a higher row index --
//     POS_i = #{j before i}     J_i = 1 + #{j before i, j a true positive}
// and stores the precision J_i / (POS_i + 1) in slot J_i - 1 of the class's list.  The counts are integers and exact.
// voc_finish_kernel, one workgroup per class: m, the number of true positives, from the tiles' counts; thread k owns slots
// [k L, k L + L) with L = ceil(m / 256); the envelope (the maximum over the later slots) crosses the threads through LDS, a
// maximum has no order; each thread adds its terms (j / n - (j - 1) / n) env_j from its highest slot down to its lowest, and
// the 256 partial sums are folded by halving.
// voc_mean_kernel: one thread adds the ap of the classes with ground truth in ascending class order.
__global__ void voc_offsets_kernel(const int64_t* __restrict__ n_gt, int C, int64_t total_gt, int64_t* __restrict__ off,
                                   int* __restrict__ flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int f = 0;
    int64_t at = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t n = n_gt[c] > 0 ? n_gt[c] : 0;
        if (n > total_gt - at) {
            off[c] = -1;                                                      // no room: the class is not scored
            f |= VOC_GT_ABOVE_TOTAL;
        } else {
            off[c] = at;
            at += n;
        }
    }
    flag[0] = f;
}

// voc_pack_kernel: thread per (row, class), classes side by side as they lie in memory.  Writes the class-major copies the
// counting streams: key[c][i] = the score of an evaluated row, -inf otherwise (so that it stands before nothing), and
// tp[c][i] = 1 for a true positive; rows are padded to whole tiles.
__global__ __launch_bounds__(THREADS) void voc_pack_kernel(const void* __restrict__ scores, int bf16, int64_t lds_,
                                                           const uint8_t* __restrict__ bytes, int64_t ldb, int64_t N, int C,
                                                           int64_t Np, float* __restrict__ key, uint8_t* __restrict__ tpT,
                                                           int* __restrict__ flag) {
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= Np * C) return;
    const int64_t i = idx / C;
    const int c = (int)(idx - i * C);
    float k = -INFINITY;
    uint8_t y = 0;
    if (i < N) {
        const int b = bytes[i * ldb + c];
        if (b != 0) {
            k = ldv(scores, i * lds_ + c, bf16);
            y = b == 2;
            if (!(fabsf(k) <= 3.402823466e38f)) atomicOr(flag, VOC_BAD_SCORE);                // NaN fails the <=
        }
    }
    key[(int64_t)c * Np + i] = k;
    tpT[(int64_t)c * Np + i] = y;
}

__global__ __launch_bounds__(THREADS) void voc_rank_kernel(const float* __restrict__ key, const uint8_t* __restrict__ tpT,
                                                           int64_t Np, int64_t tiles, const int64_t* __restrict__ n_gt,
                                                           const int64_t* __restrict__ off, double* __restrict__ prec,
                                                           int* __restrict__ tp_part, int* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) float s_s[THREADS];
    __shared__ __attribute__((aligned(16))) int s_b[THREADS];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int c = blockIdx.y;
    const float* kc = key + (int64_t)c * Np;
    const uint8_t* yc = tpT + (int64_t)c * Np;
    if (tid == 0) s_n = 0;
    const float si = kc[t * THREADS + tid];
    const int tp = yc[t * THREADS + tid];
    const int any_tp = __syncthreads_or(tp);                                  // also orders the store to s_n
    if (tp) atomicAdd(&s_n, 1);
    __syncthreads();
    if (tid == 0) tp_part[(int64_t)c * tiles + t] = s_n;
    if (!any_tp) return;
    const bool wave_counts = __any(tp);
    int pos = 0, jm1 = 0;                                                     // N < 2^31
    for (int64_t tb = 0; tb < tiles; ++tb) {
        __syncthreads();                                                      // the previous tile has been read
        s_s[tid] = kc[tb * THREADS + tid];
        s_b[tid] = yc[tb * THREADS + tid];
        __syncthreads();
        if (!wave_counts) continue;
        if (tb == t) {                                                        // the own tile: equal scores by row index
            for (int k = 0; k < THREADS; ++k) {
                const float sj = s_s[k];
                const int before = (sj > si) | ((sj == si) & (k > tid));
                pos += before;
                jm1 += before & s_b[k];
            }
        } else if (tb > t) {                                                  // later rows: an equal score stands before
            for (int k = 0; k < THREADS; k += 4) {
                const float4 s4 = *reinterpret_cast<const float4*>(&s_s[k]);
                const int4 y4 = *reinterpret_cast<const int4*>(&s_b[k]);
                const int g0 = s4.x >= si, g1 = s4.y >= si, g2 = s4.z >= si, g3 = s4.w >= si;
                pos += g0 + g1 + g2 + g3;
                jm1 += (g0 & y4.x) + (g1 & y4.y) + (g2 & y4.z) + (g3 & y4.w);
            }
        } else {                                                              // earlier rows: only a higher score does
            for (int k = 0; k < THREADS; k += 4) {
                const float4 s4 = *reinterpret_cast<const float4*>(&s_s[k]);
                const int4 y4 = *reinterpret_cast<const int4*>(&s_b[k]);
                const int g0 = s4.x > si, g1 = s4.y > si, g2 = s4.z > si, g3 = s4.w > si;
                pos += g0 + g1 + g2 + g3;
                jm1 += (g0 & y4.x) + (g1 & y4.y) + (g2 & y4.z) + (g3 & y4.w);
            }
        }
    }
    if (!tp) return;
    const int64_t n = n_gt[c], o = off[c];
    if (jm1 >= n) {
        if (n > 0) atomicOr(flag, VOC_TP_ABOVE_GT);                           // the reference raises ValueError here;
        return;                                                               // a class without ground truth it never scores
    }
    if (o >= 0) prec[o + jm1] = (double)(jm1 + 1) / (double)(pos + 1);
}

__global__ __launch_bounds__(THREADS) void voc_finish_kernel(int64_t tiles, const int64_t* __restrict__ n_gt,
                                                             const int64_t* __restrict__ off, const double* __restrict__ prec,
                                                             const int* __restrict__ tp_part, double* __restrict__ ap) {
    __shared__ double s_d[THREADS];
    __shared__ long long s_m[THREADS];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int64_t n = n_gt[c], o = off[c];
    long long cnt = 0;
    for (int64_t t = tid; t < tiles; t += THREADS) cnt += tp_part[(int64_t)c * tiles + t];
    s_m[tid] = cnt;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) s_m[tid] += s_m[tid + h];
        __syncthreads();
    }
    const int64_t m = s_m[0];
    if (n <= 0 || m > n || o < 0) {                                           // no ground truth: NaN; the two flagged cases too
        if (tid == 0) ap[c] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int64_t L = (m + THREADS - 1) / THREADS;
    const int64_t a = (int64_t)tid * L < m ? (int64_t)tid * L : m;
    const int64_t b = a + L < m ? a + L : m;
    double mx = 0.0;                                                          // precisions are positive
    for (int64_t j = a; j < b; ++j) mx = fmax(mx, prec[o + j]);
    s_d[tid] = mx;
    __syncthreads();
    double env = 0.0;                                                         // the maximum over the slots of the later threads
    for (int k = tid + 1; k < THREADS; ++k) env = fmax(env, s_d[k]);
    __syncthreads();
    double acc = 0.0;
    for (int64_t j = b - 1; j >= a; --j) {
        env = fmax(env, prec[o + j]);
        const double step = (double)(j + 1) / (double)n - (double)j / (double)n;
        acc = acc + step * env;
    }
    s_d[tid] = acc;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) s_d[tid] = s_d[tid] + s_d[tid + h];
        __syncthreads();
    }
    if (tid == 0) ap[c] = s_d[0];
}

__global__ void voc_mean_kernel(int C, const int64_t* __restrict__ n_gt, const double* __restrict__ ap,
                                double* __restrict__ summary) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0;
    int64_t kept = 0;
    for (int c = 0; c < C; ++c) {
        const double v = ap[c];
        if (n_gt[c] > 0 && v == v) {
            sum = sum + v;
            ++kept;
        }
    }
    summary[0] = kept > 0 ? sum / (double)kept : __longlong_as_double(0x7ff8000000000000ll);
    summary[1] = (double)kept;
}

}  // namespace

extern "C" int focus_ava_match(const float* boxes, int64_t K, int C, const int64_t* grp_off, const int64_t* det_rows,
                               const int64_t* grp_image, int64_t n_groups, const int64_t* gt_off, const int32_t* gt_class,
                               const double* gt_boxes, int64_t n_images, const uint8_t* whitelist, uint8_t* out, int64_t ldo,
                               int64_t* counts, int32_t* flag, void* stream) {
    if (!out || !counts || !flag || !whitelist) return FOCUS_ERR_NULL;
    if (K > 0 && (!boxes || !grp_off || !det_rows || !grp_image)) return FOCUS_ERR_NULL;
    if (n_images > 0 && (!gt_off || !gt_class || !gt_boxes)) return FOCUS_ERR_NULL;
    if (K < 0 || C < 1 || C > 65535 * THREADS || n_groups < 0 || n_groups > 2147483647ll || n_images < 0 || ldo < C)
        return FOCUS_ERR_SHAPE;
    if (K == 0 || n_groups == 0) return FOCUS_OK;                             // nothing is written: the caller's zeros stand
    ava_match_kernel<<<dim3((unsigned)n_groups, (unsigned)cdiv64(C, THREADS)), THREADS, 0, (hipStream_t)stream>>>(
        boxes, K, C, grp_off, det_rows, grp_image, n_images, gt_off, gt_class, gt_boxes, whitelist, out, ldo,
        reinterpret_cast<unsigned long long*>(counts), flag);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" size_t focus_voc_ap_workspace_bytes(int64_t N, int C, int64_t total_gt) {
    if (N < 0 || C < 1 || total_gt < 0) return 0;
    const size_t tiles = (size_t)cdiv64(N, THREADS);
    const size_t parts = (tiles * (size_t)C * 4 + 7) / 8 * 8;
    const size_t packed = tiles * THREADS * (size_t)C;                        // a float key and a byte mark per padded (row, class)
    return (size_t)total_gt * 8 + (size_t)C * 8 + parts + packed * 4 + (packed + 7) / 8 * 8 + 8;
}

extern "C" int focus_voc_ap(const void* scores, int dtype, int64_t lds, const uint8_t* bytes, int64_t ldb, int64_t N, int C,
                            const int64_t* n_gt, int64_t total_gt, double* ap, double* summary, int32_t* flag, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!n_gt || !ap || !summary || !flag || !workspace) return FOCUS_ERR_NULL;
    if (N > 0 && (!scores || !bytes)) return FOCUS_ERR_NULL;
    if (N < 0 || C < 1 || C > 65535 || total_gt < 0 || lds < C || ldb < C) return FOCUS_ERR_SHAPE;
    const int64_t tiles = cdiv64(N, THREADS);
    if (N > 2147483647ll - THREADS || tiles * C > 2147483647ll) return FOCUS_ERR_SHAPE;      // 32-bit ranks; the packing grid
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (!focus_aligned(workspace, 8)) return FOCUS_ERR_ALIGN;
    if (workspace_bytes < focus_voc_ap_workspace_bytes(N, C, total_gt)) return FOCUS_ERR_WORKSPACE;
    double* prec = reinterpret_cast<double*>(workspace);
    int64_t* off = reinterpret_cast<int64_t*>(prec + total_gt);
    int* tp_part = reinterpret_cast<int*>(off + C);
    const int64_t Np = tiles * THREADS;
    float* key = reinterpret_cast<float*>(reinterpret_cast<char*>(tp_part) + ((size_t)tiles * (size_t)C * 4 + 7) / 8 * 8);
    uint8_t* tpT = reinterpret_cast<uint8_t*>(key + Np * C);
    hipStream_t s = (hipStream_t)stream;
    voc_offsets_kernel<<<dim3(1), 64, 0, s>>>(n_gt, C, total_gt, off, flag);
    FOCUS_CHECK_LAUNCH();
    if (N > 0) {
        voc_pack_kernel<<<dim3((unsigned)cdiv64(Np * C, THREADS)), THREADS, 0, s>>>(scores, dtype == FOCUS_BF16, lds, bytes, ldb, N,
                                                                                    C, Np, key, tpT, flag);
        FOCUS_CHECK_LAUNCH();
        voc_rank_kernel<<<dim3((unsigned)tiles, (unsigned)C), THREADS, 0, s>>>(key, tpT, Np, tiles, n_gt, off, prec, tp_part, flag);
        FOCUS_CHECK_LAUNCH();
    }
    voc_finish_kernel<<<dim3((unsigned)C), THREADS, 0, s>>>(tiles, n_gt, off, prec, tp_part, ap);
    FOCUS_CHECK_LAUNCH();
    voc_mean_kernel<<<dim3(1), 64, 0, s>>>(C, n_gt, ap, summary);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
