/*
 * include/focus_amd.h -- C ABI of libfocus_amd.so (MI355X / gfx950 hot path of srv902/FOCUS).
 *
 * The reference has no FFI: its operator surface is the Python module API.
 * Each entry point below replaces the device work done by the cited reference call site; the
 * Python host mirror (focus_amd/slowfast/...) keeps the reference's signatures and calls these
 * through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); nothing here allocates,
 *     frees or synchronises; kernels are enqueued on `stream` (a hipStream_t, may be NULL);
 *   - tensors are dense row-major in the documented shape unless strides are passed;
 *   - `dtype` selects activation/weight storage: FOCUS_F32 or FOCUS_BF16 (accumulation, softmax and
 *     normalisation statistics are always fp32); LayerNorm affine parameters, biases and all
 *     parameter gradients are fp32 in both modes;
 *   - return value: 0 on success, negative focus_status on error (focus_strerror() names it).
 */
#ifndef FOCUS_AMD_H
#define FOCUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum focus_dtype { FOCUS_F32 = 0, FOCUS_BF16 = 1, FOCUS_FP8_E4M3 = 2 /* OCP e4m3fn codes: weights (B of focus_gemm), or both operands of focus_gemm_mx */ };

enum focus_status {
    FOCUS_OK = 0,
    FOCUS_ERR_SHAPE = -1,      /* inconsistent or unsupported shape            */
    FOCUS_ERR_DTYPE = -2,      /* unsupported dtype combination                */
    FOCUS_ERR_ALIGN = -3,      /* pointer / stride alignment not met           */
    FOCUS_ERR_LAUNCH = -4,     /* hipGetLastError() reported a launch failure  */
    FOCUS_ERR_NULL = -5,       /* required pointer is NULL                     */
    FOCUS_ERR_WORKSPACE = -6   /* workspace too small                          */
};

const char* focus_strerror(int status);
/* ABI version of this library (bumped on any signature change). */
int focus_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C = epi(alpha * A.B [+ bias]) [+ residual]      (fp32 accumulate)
 * Replaces every nn.Linear / bmm / einsum contraction on the path (attention.py:506,524-529,536-537,
 * 555; common.py:26-34; orvit.py:59-72; steve.py:61-62,75-76,83; stem_helper.py:318 as im2col GEMM)
 * and their autograd backward.  A is [M,K], B is [K,N], C is [M,N]; all three are addressed by
 * element strides (rs = row stride, cs = column stride) and a two-level batch (batch0 x batch1).
 * The MFMA path is taken when dtype is bf16 and both A and B are contiguous along K (csA==1,
 * rsB==1), 16-byte aligned; everything else runs the generic tiled kernel.
 * Degenerate sizes (pinned by tests/test_gpu_gemm_desc.py): M <= 0 or N <= 0 returns FOCUS_OK without a launch and
 * leaves C and aux alone; K == 0 is an empty sum, C = epi(bias) [+ residual] [+ C] (generic kernel; with GELU the
 * pre-activation saved in aux is the bias); K < 0 is FOCUS_ERR_SHAPE.  Nothing outside the batch0 x batch1 windows
 * of M x N elements of C (and of aux, for GELU) is written.
 * ----------------------------------------------------------------------------------------------*/
enum focus_epilogue {
    FOCUS_EPI_NONE = 0,
    FOCUS_EPI_GELU = 1,    /* C = gelu_erf(v); if aux != NULL the pre-activation v is stored in aux */
    FOCUS_EPI_RELU = 2,
    FOCUS_EPI_TANH = 3,
    FOCUS_EPI_DGELU = 4,   /* C = v * gelu'(aux)      aux = saved pre-activation                    */
    FOCUS_EPI_DRELU = 5,   /* C = v * (aux > 0)       aux = saved output                            */
    FOCUS_EPI_DTANH = 6    /* C = v * (1 - aux^2)     aux = saved output                            */
};

typedef struct focus_gemm_desc {
    int32_t M, N, K;
    int32_t batch0, batch1;
    const void* A; int64_t rsA, csA, bsA0, bsA1;
    const void* B; int64_t rsB, csB, bsB0, bsB1;
    void* C;       int64_t rsC, csC, bsC0, bsC1;
    const float* bias;        /* [N] fp32 or NULL (applied before the activation)                   */
    const void* residual;     /* same dtype/strides as C, added after the activation, or NULL       */
    void* aux;                /* same dtype/strides as C; see focus_epilogue                        */
    float alpha;
    int32_t accumulate;       /* 1: C += result (C must be fp32)                                    */
    int32_t epilogue;         /* enum focus_epilogue                                                */
    int32_t dtype_ab;         /* storage of A and B                                                 */
    int32_t dtype_c;          /* storage of C, residual and aux                                     */
    int32_t dtype_b;          /* 0: B is stored like A.  FOCUS_FP8_E4M3: B holds e4m3 codes (1 byte per element,
                                 strides in elements), A is bf16: the "fp8 weights, bf16 activations" GEMM     */
    int32_t pad_;
    const float* b_scale;     /* DEVICE scalar: the per-tensor scale of an fp8 B (C = epi(alpha * b_scale * A.B ...)) */
} focus_gemm_desc;

int focus_gemm(const focus_gemm_desc* desc, void* stream);

/* Kernel family the last focus_gemm() call of this thread dispatched to (measurement attribution only). */
enum focus_gemm_kernel {
    FOCUS_GEMM_KERNEL_GENERIC = 0,   /* gemm_generic.hip (fp32 / odd strides)                       */
    FOCUS_GEMM_KERNEL_NT = 1,        /* gemm_mfma.hip uniform 128x128 (few tiles, split-K)          */
    FOCUS_GEMM_KERNEL_NT_WS = 2,     /* gemm_mfma_ws.hip wave-specialised (the step's dominant kernel) */
    FOCUS_GEMM_KERNEL_TN = 3,        /* gemm_mfma_tn*.hip (weight gradients)                        */
    FOCUS_GEMM_KERNEL_NT_SMALL = 4,  /* gemm_mfma_small.hip (M <= 1024 rows: recurrent / motion-stream Linears) */
    FOCUS_GEMM_KERNEL_NT_MX = 5      /* gemm_mx_fp8.hip (focus_gemm_mx: MX-scaled e4m3 activations x e4m3 weights) */
};
int focus_gemm_last_kernel(void);

/* Tuning hook: force the row-tile height of the wave-specialised NT kernel (128 or 192; 0 = automatic choice by the
 * modelled rounds-x-tile-time cost).  Used by tools/gemm_tile_ab.py for A/B timing inside one process. */
int focus_gemm_tile_override(int bm);

/* MX e4m3 activations (TRAIN.FP8_ACTIVATIONS): x [rows, cols] bf16 -> codes [rows, cols] OCP e4m3 + scales
 * [rows, cols / 32] E8M0, one per block of 32 consecutive elements of a row.  Block amax = 1.m x 2^E:
 * e = E - 8 + (m > 0.75) (the smallest e with amax <= 448 x 2^e), clamped to [-127, 127], -127 for an all-zero block;
 * scale byte = e + 127, 0xFF for a block holding a NaN or an Inf (its codes are unspecified); code = RNE_e4m3(x * 2^-e)
 * in fp32.  dtype must be FOCUS_BF16; cols % 32 == 0; strides in elements (x) and bytes (codes, scales): ldx % 8,
 * ld_codes % 16, ld_scales % 4 == 0; x and codes 16-byte, scales 4-byte aligned. */
int focus_mx_quant(const void* x, int64_t ldx, int rows, int cols, int dtype, void* codes, int64_t ld_codes, void* scales,
                   int64_t ld_scales, void* stream);

/* MX-scaled fp8 NT GEMM (gemm_mx_fp8.hip, v_mfma_scale_f32_16x16x128_f8f6f4):
 *   C = epi(alpha * b_scale * sum_k dec(A[m,k]) 2^(a_scales[m, k/32] - 127) dec(B[k,n]) + bias) [+ residual]
 * A: focus_mx_quant codes [M,K] (dtype_ab = FOCUS_FP8_E4M3, csA = 1, rsA % 16 == 0); a_scales: its E8M0 bytes
 * [M, K/32] at row stride ld_a_scales (bytes, % 4 == 0); B: e4m3 weight codes given as [N,K] rows (dtype_b =
 * FOCUS_FP8_E4M3, rsB = 1, csB % 16 == 0) with the per-tensor DEVICE scalar b_scale; C, residual, aux bf16 (csC = 1).
 * batch 1, N % 64 == 0, K % 128 == 0, any M; epilogue NONE, GELU (pre-activation to aux if given) or RELU. */
int focus_gemm_mx(const focus_gemm_desc* desc, const void* a_scales, int64_t ld_a_scales, void* stream);

/* Weight-gradient form (A strided along the reduction: rsA == 1, csB == 1, bf16 in, fp32 out): the long reduction is
 * split over workgroups.  With desc->aux == NULL the partial sums are added to a zero-initialised C with fp32
 * atomics (desc->accumulate must be 1); with desc->aux pointing to focus_gemm_tn_workspace_bytes(M, N, K) bytes the
 * partials are stored to per-split slabs and summed by a second kernel (no atomics, bitwise reproducible, C is
 * overwritten). */
size_t focus_gemm_tn_workspace_bytes(int M, int N, int K);
/* Batched form (desc->batch0 == 1, batch1 = batch independent products whose outputs are stacked densely:
 * rsC == N, bsC1 == M*N; operands offset by bsA1 / bsB1 per batch): slab mode only, aux of this many bytes. */
size_t focus_gemm_tn_batched_workspace_bytes(int M, int N, int K, int batch);

/* nn.Linear backward w.r.t. its parameters in one pass over dy (replaces autograd's dy^T @ x and dy.sum(0) of
 * common.py:26-34 / attention.py:506,536-537,555):  dw[N,K] = dy[M,N]^T . x[M,K],  db[N] = sum_m dy[m,:]  (db may be
 * NULL).  bf16 operands, fp32 results, both overwritten.  The column sums ride on the matrix pipe of the
 * weight-gradient kernel (ones^T . dy) when the wave-specialised kernel takes the shape; otherwise focus_colsum runs.
 * ws: focus_linear_wgrad_workspace_bytes(N, K, M) bytes.  N % 8 == 0, K % 8 == 0, 16-byte aligned rows. */
size_t focus_linear_wgrad_workspace_bytes(int N, int K, int M);
int focus_linear_wgrad(const void* dy, const void* x, float* dw, float* db, void* ws, size_t ws_bytes, int M, int N,
                       int K, int64_t ld_dy, int64_t ld_x, int dtype, void* stream);

/* y[M,N] = act(x[M,K] . w[N,K]^T + bias) + residual -- nn.Linear forward (thin wrapper over focus_gemm). */
int focus_linear_fwd(const void* x, const void* w, const float* bias, const void* residual, void* y,
                     void* aux, int M, int N, int K, int epilogue, int dtype, void* stream);

/* out[n] (+)= sum_m x[m,n]   (bias gradients)  x is `dtype`, out fp32.  */
int focus_colsum(const void* x, float* out, int M, int N, int64_t row_stride, int accumulate, int dtype,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the last axis (video_model_builder.py:1129 eps 1e-6; steve.py:35-37 eps 1e-5).
 * ----------------------------------------------------------------------------------------------*/
int focus_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                        float* rstd, int rows, int D, float eps, int dtype, void* stream);
/* dgamma/dbeta are written (not accumulated); `partial` is a [2, nblk, D] fp32 scratch with
 * nblk = focus_layernorm_bwd_blocks(rows).  dres (may be NULL): gradient arriving on the residual path around a
 * pre-norm block (x -> x + f(LN(x)), attention.py:116-126); it is added into dx in the same pass, replacing the
 * separate accumulation autograd would do.  dgamma == dbeta == NULL: only `partial` is written -- partial[0] holds nblk row
 * vectors whose sum is dgamma, partial[1] likewise dbeta -- for a caller that applies the same LayerNorm many times and
 * reduces all applications' partials in one pass at the end (STEVE's slot loop: 213 applications per step).
 *
 * Statuses of the four entry points below, judged in this order before any launch; a refused call writes nothing
 * (pinned by tests/test_ln_ref_cpu.py and tests/test_gpu_layernorm.py):
 *   FOCUS_ERR_NULL   gamma, beta (forward) or partial (backward) is NULL; a row-sized buffer (x, y, mean, rstd, dy, dx) is
 *                    NULL while rows > 0; dgamma without dbeta or the reverse.
 *   FOCUS_ERR_SHAPE  D <= 0, D % 4 != 0, D > 4096, rows_per_block <= 0, block_stride % 4 != 0, rows < 0 (backward).
 *   FOCUS_ERR_ALIGN  x, y, dy, dx or a non-NULL dres not aligned to 4 elements of `dtype` (16 bytes fp32, 8 bytes bf16), or
 *                    gamma / beta not to 16 bytes.
 *   FOCUS_OK         rows == 0 included: the forward does nothing (rows <= 0, before the shape is judged); the backward
 *                    zero-fills dgamma and dbeta when given and partial[2][1][D] (focus_layernorm_bwd_blocks(0) == 1) on
 *                    the stream.  With rows == 0 the row-sized buffers may be NULL: an empty tensor has no address. */
int focus_layernorm_bwd_blocks(int rows);
int focus_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                        const float* rstd, const void* dres, void* dx, float* dgamma, float* dbeta, float* partial,
                        int rows, int D, int dtype, void* stream);
/* The same two kernels over ROW BLOCKS: x (and, backward, dx) is a set of blocks of rows_per_block dense rows whose
 * starts are block_stride elements apart -- frame t of a [B,T,N,D] video tensor read and differentiated in place (pointer
 * to frame t, rows_per_block = N, block_stride = T*N*D, rows = B*N): no per-frame copies either way (steve.py:60, :68).
 * y, dy, mean, rstd are dense [rows, D]. */
int focus_layernorm_fwd_blocks(const void* x, int rows_per_block, int64_t block_stride, const float* gamma,
                               const float* beta, void* y, float* mean, float* rstd, int rows, int D, float eps, int dtype,
                               void* stream);
int focus_layernorm_bwd_blocks_strided(const void* dy, const void* x, int rows_per_block, int64_t block_stride,
                                       const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                       float* dbeta, float* partial, int rows, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row softmax over segments:  x viewed as [rows, L] with row stride `stride`; in place allowed.
 * bwd: dx = y * (dy - sum(dy*y)).   Used by the fp32 (unfused) attention path, the motion-stream
 * joint attention (attention.py:380-381), the cls row (attention.py:436-440) and the slot predictor
 * (transformer.py:44).
 * ----------------------------------------------------------------------------------------------*/
int focus_softmax_fwd(const void* x, void* y, int64_t rows, int L, int64_t stride, float scale, int dtype,
                      void* stream);
int focus_softmax_bwd(const void* dy, const void* y, void* dx, int64_t rows, int L, int64_t stride,
                      float scale, int dtype, void* stream);
/* Causal variant (STEVE/transformer.py:145-166, self_attn_mask = triu(1)): row r sees columns 0 .. r % period, the
 * masked tail of y is exact zeros; its backward is focus_softmax_bwd. */
int focus_softmax_causal_fwd(const void* x, void* y, int64_t rows, int L, int64_t stride, int period, float scale,
                             int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Trajectory attention (attention.py:499-557).  qkv is the output of the fused qkv Linear,
 * [B, N, 3C] with N = 1 + F*P, channel order (q|k|v) x (head, d).
 *   space step (:514-535): cls_out [B,C]; xt = x~ [B,S,F,C]; xdiag [B,S,C]; lse [B,h,S,F] and
 *   cls_lse [B,h] (fp32, saved for backward).
 *   time step (:538-549, use_original_code=True): q2 [B,S,C] (un-scaled proj_q output),
 *   k2 [B,S,F,C], xt -> out [B,S,C]; attn2 [B,h,S,F] fp32 saved for backward.
 * Workspace sizes are returned by the *_workspace_bytes queries (0 when none is needed).
 * ----------------------------------------------------------------------------------------------*/
size_t focus_traj_space_workspace_bytes(int B, int F, int P, int heads, int d, int dtype, int backward);
int focus_traj_space_fwd(const void* qkv, void* xt, void* xdiag, void* cls_out, float* lse, float* cls_lse,
                         void* workspace, size_t workspace_bytes, int B, int F, int P, int heads, int d,
                         int dtype, void* stream);
/* dqkv [B,N,3C] is fully written. dxt / dxdiag / dcls are the cotangents of xt / xdiag / cls_out.
 * The route is decided from the whole shape, the same way by the workspace query, the forward and the backward: the fused
 * kernels take bf16, d = 64, P <= 448 and F <= 16, everything else the generic path.  On the fused route qkv, xt, xdiag
 * (forward) and qkv, xt, dxt, dxdiag, dqkv and the workspace (backward) must be 16-byte aligned: FOCUS_ERR_ALIGN before
 * anything is launched. */
int focus_traj_space_bwd(const void* qkv, const void* xt, const void* cls_out, const float* lse,
                         const float* cls_lse, const void* dxt, const void* dxdiag, const void* dcls,
                         void* dqkv, void* workspace, size_t workspace_bytes, int B, int F, int P,
                         int heads, int d, int dtype, void* stream);
/* out_bstride / dout_bstride: elements between consecutive batches of out / dout (S*C when dense; (S+1)*C when the
 * rows live in tokens 1.. of a [B,1+S,C] buffer whose token 0 is the cls row -- saves the concatenation of
 * attention.py:551 and the slice copy of its backward). */
int focus_traj_time_fwd(const void* q2, const void* k2, const void* xt, void* out, int64_t out_bstride, float* attn2,
                        int B, int S, int F, int heads, int d, int dtype, void* stream);
int focus_traj_time_bwd(const void* q2, const void* k2, const void* xt, const float* attn2, const void* dout,
                        int64_t dout_bstride, void* dq2, void* dk2, void* dxt, int dxt_accumulate, int B, int S, int F,
                        int heads, int d, int dtype, void* stream);

/* Temporal step WITHOUT k2 = proj_kv(x~)[:, :C] in HBM (attention.py:536-549, use_original_code=True).  The logits are
 *   scale * q2[s,h,:] . (Wk[h] x~[s,f,:] + bk[h])  =  scale * (Wk[h]^T q2[s,h,:]) . x~[s,f,:]  + (a term constant in f),
 * and the softmax over f is shift invariant, so k2 [B,S,F,C] (the block's largest GEMM: 8x the tokens) and dk2 are
 * never formed; u[s,h,:] = Wk[h]^T q2[s,h,:] is produced per 64-channel chunk on chip (csrc/traj_time2.hip).
 * bf16, head dim 64, heads <= 16, F in {4, 8, 16}.  wkT: [C rows (input channel c)][ldw] bf16 whose columns 0..C-1 hold
 * Wk^T (the transposed shadow of proj_kv.weight).  q2 [B,S,C] is the UN-scaled proj_q output.
 *   fwd: out rows [B,S,C] at batch stride out_bstride (see focus_traj_time_fwd); attn2 [B,S,h,F] fp32 (saved);
 *        ws: focus_traj_time2_workspace_bytes() bytes of scratch.
 *   bwd: dxt [B,S,F,C] (fully written: a*dout + sum_h dl*u); g [h,B*S,C] bf16 = d(loss)/d(u), head-major so that each
 *        head's slice is a dense matrix, from which the caller forms  dq2[:, h*64+dd] = sum_c g[h,:,c] Wk[h*64+dd, c]
 *        and  dWk[h*64+dd, c] = sum_s q2[s,h*64+dd] g[h,s,c]  (two batched GEMMs over the heads); dl [B,S,F,16] bf16 scratch
 *        (columns heads..15 are written as +0).  proj_kv.bias gets its exact zero gradient.
 * Status, judged in this order before any launch (pinned by tests/test_gpu_traj_time2.py; a refused call writes nothing):
 *   FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE (B <= 0, S <= 0, F not in {4, 8, 16}, heads outside 1..16, d != 64, a
 *   dtype other than FOCUS_BF16, ldw < C, ldw % 8 != 0, a batch stride below S*C or not a multiple of 8);
 *   FOCUS_ERR_ALIGN (a pointer not 16-byte aligned); FOCUS_ERR_WORKSPACE (fwd: ws_bytes below
 *   focus_traj_time2_workspace_bytes(), which is 0 for a non-positive size or d != 64). */
size_t focus_traj_time2_workspace_bytes(int B, int S, int F, int heads, int d);
int focus_traj_time2_fwd(const void* q2, const void* xt, const void* wkT, int64_t ldw, void* out, int64_t out_bstride,
                         float* attn2, void* ws, size_t ws_bytes, int B, int S, int F, int heads, int d, int dtype,
                         void* stream);
int focus_traj_time2_bwd(const void* q2, const void* xt, const void* wkT, int64_t ldw, const float* attn2,
                         const void* dout, int64_t dout_bstride, void* dxt, void* g, void* dl, int B, int S, int F,
                         int heads, int d, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RoIAlign over patch-token feature maps (ORViT/utils.py:58-75 -> torchvision.ops.roi_align with
 * output_size=(H,W), sampling_ratio=-1, aligned=True).  Channels-last on both sides:
 *   feat  image i = (b, t) = (i / imgs_per_batch, i % imgs_per_batch) starts at feat + b*batch_stride + t*img_stride
 *         (elements): the tokens are read in place from the residual stream [B,1+T*H*W,C] (pointer to token 1,
 *         img_stride = H*W*C, imgs_per_batch = T, batch_stride = (1+T*H*W)*C); a dense [NI,H*W,C] map is
 *         imgs_per_batch = NI, img_stride = H*W*C;
 *   rois  [K,4] fp32 xyxy in input pixels, roi_img [K] int32 image index;
 *   out   [K, PH*PW, C].
 * The integer side (sampling grid size, neighbour indices) is bit-exact with oracle/roi_align_ref.c.
 * ----------------------------------------------------------------------------------------------*/
int focus_roi_align_fwd(const void* feat, int64_t img_stride, int imgs_per_batch, int64_t batch_stride,
                        const float* rois, const int32_t* roi_img, void* out, int NI, int C, int H, int W, int K,
                        int PH, int PW, float spatial_scale, int sampling_ratio, int aligned, int relu, int dtype,
                        void* stream);
/* dfeat: image maps addressed like feat, `dtype`, every map fully written (no zero-initialisation needed; rows between
 * the maps -- the cls row of a token buffer -- are not touched).  Maps up to 16x16 with up to
 * 14x14 bins use the separable form dfeat = sum_rois Ay . dout . Ax^T (no atomics, accumulators in registers); other
 * shapes go through fp32 atomics into `ws` (focus_roi_align_bwd_workspace_bytes, 0 for the separable path) + a cast
 * and need the dense addressing (FOCUS_ERR_SHAPE otherwise).
 * relu != 0 (forward): out = max(RoIAlign, 0) -- the ReLU that follows when patch_to_d's first Linear is applied BEFORE
 * sampling (it has no bias, so it commutes with the bilinear sampling: SURVEY a10); relu_out (backward, may be NULL,
 * separable path only): that saved output, used as the ReLU mask on dout. */
size_t focus_roi_align_bwd_workspace_bytes(int NI, int C, int H, int W, int PH, int PW);
int focus_roi_align_bwd(const void* dout, const void* relu_out, const float* rois, const int32_t* roi_img, void* dfeat, int64_t img_stride,
                        int imgs_per_batch, int64_t batch_stride, void* ws, size_t ws_bytes, int NI, int C, int H, int W, int K, int PH, int PW, float spatial_scale,
                        int sampling_ratio, int aligned, int dtype, void* stream);
/* Debug/parity export of the integer side: grid [K,2], nbr [K,PH,PW,4] (int32). */
int focus_roi_align_indices(const float* rois, int32_t* grid, int32_t* nbr, int H, int W, int K, int PH,
                            int PW, float spatial_scale, int sampling_ratio, int aligned, void* stream);

/* max over the cells of each RoI (orvit.py:138): x [K, cells, C] -> y [K, C], arg [K, C] int32. */
int focus_cell_amax_fwd(const void* x, void* y, int32_t* arg, int K, int cells, int C, int dtype,
                        void* stream);
/* dx [K, cells, C] is fully written (zeros except the arg-max cell). */
int focus_cell_amax_bwd(const void* dy, const int32_t* arg, void* dx, int K, int cells, int C, int dtype,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * RoI head pooling (head_helper.py:103-118: AvgPool3d([T,1,1]) -> ROIAlign(resolution, 1/scale_factor, sampling_ratio=0,
 * aligned) -> MaxPool2d(resolution)) over the token stream, without the [B,C,T,H,W] transpose and without the
 * [K, PH*PW, C] RoIAlign output:
 *     pooled[k, c] = max over bins (ph, pw) of RoIAlign(mean_t x[b_k, t, :, :, c])
 *   x       patch tokens [B, T*H*W, C] read in place: pointer to the first patch token of sample 0, sample b at
 *           x + b*batch_stride elements (the stream [B, cls + T*H*W, C]: pointer to token `cls`, batch_stride =
 *           (cls + T*H*W)*C); `dtype`;
 *   rois    [K,5] fp32 (batch index, x1, y1, x2, y2), the box in input pixels -- the reference's meta["boxes"].  Boxes come
 *           in any order of batch index.  A batch index that is not an integer in [0, B) is the caller's error (the Python
 *           side refuses it on the host); the kernels read and write nothing for such a box: pooled = 0, arg = 0, no gradient;
 *   pooled  [K,C] `dtype`; arg [K,C] int32 = ph*PW + pw of the winning bin, the lowest index among equal bins;
 *   ws      fp32 [B, H*W, C] (focus_roi_head_workspace_bytes, 16-byte aligned): the temporal mean, summed over t in order.
 * RoIAlign is torchvision's: the -0.5 shift and no clamp of the box size to 1 when `aligned`, sampling_ratio <= 0 = adaptive
 * grid ceil(roi / bins), count = max(grid_h*grid_w, 1), samples outside [-1,H] x [-1,W] contribute 0, edges clamped; grid
 * sizes and neighbour indices are those of focus_roi_align_indices.  Accumulation is fp32.  A box that samples nothing (all
 * outside, or an empty grid) gives pooled = 0, arg = 0.
 * backward: dx addressed like x; every patch-token row of every sample is written (samples without boxes: zeros), rows
 *   between the samples (the cls row) are not touched.  d(k,c) flows through the bilinear weights of bin arg[k,c], divided by
 *   count and by T, the same for every t.  No atomics: one workgroup owns an (image, channel chunk) slab and adds the boxes
 *   in index order, so two runs on the same inputs are bit-equal.
 * Status: K == 0 is FOCUS_OK (forward: nothing written; backward: dx = 0).  FOCUS_ERR_DTYPE unless fp32 / bf16;
 *   FOCUS_ERR_ALIGN unless C % 4 == 0, batch_stride % 4 == 0 and x / dx aligned to 4 elements; FOCUS_ERR_SHAPE for
 *   T > 1024, PH*PW > 1024, H*W > 512 (the backward slab lives in LDS), K or B > 65535, batch_stride < T*H*W*C or any
 *   non-positive size; FOCUS_ERR_WORKSPACE for a short or misaligned ws.
 * ----------------------------------------------------------------------------------------------*/
size_t focus_roi_head_workspace_bytes(int B, int H, int W, int C);
int focus_roi_head_fwd(const void* x, int64_t batch_stride, const float* rois, void* pooled, int32_t* arg, void* ws,
                       size_t ws_bytes, int B, int T, int H, int W, int C, int K, int PH, int PW, float spatial_scale,
                       int sampling_ratio, int aligned, int dtype, void* stream);
int focus_roi_head_bwd(const void* dpooled, const int32_t* arg, const float* rois, void* dx, int64_t batch_stride, int B,
                       int T, int H, int W, int C, int K, int PH, int PW, float spatial_scale, int sampling_ratio,
                       int aligned, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ORViT token plumbing (ORViT/orvit.py:145-147, :152-157, :165-169), one pass each way instead of cat / slice / add chains.
 * x   [B, 1+T*HW, C]     residual stream (cls row + patch tokens)
 * obj [B, T, O, C]       object tokens
 * all [B, 1+T*(HW+O), C] cls row, then per frame its HW patch tokens followed by its O object tokens
 * assemble: all = cat(cls, cat(patch.view(B,T,HW,C), obj, dim=2).flatten(1,2)); the adjoint scatters d(all) into
 *           dx (every row written) and dobj.  Pure row copies: any dtype, C * elem_size % 16 == 0.
 * merge:    out[b,0] = x[b,0] + s_b*y[b,0];  out[b,1+t*HW+p] = x[..] + s_b*(y[b,1+t*(HW+O)+p] + mm[b,t*HW+p])
 *           (y = attention output over `all`, mm = motion-stream MLP output or NULL, s = per-sample stochastic-depth
 *           scale or NULL for 1); adjoint: dy (object rows zero), dmm = s*dout[:,1:] (or NULL); dx is dout itself.
 * ----------------------------------------------------------------------------------------------*/
int focus_orvit_assemble(const void* x, const void* obj, void* all, int B, int T, int HW, int O, int C, int dtype,
                         void* stream);
int focus_orvit_assemble_bwd(const void* dall, void* dx, void* dobj, int B, int T, int HW, int O, int C, int dtype,
                             void* stream);
int focus_orvit_merge(const void* x, const void* y, const void* mm, const float* scale, void* out, int B, int T, int HW,
                      int O, int C, int dtype, void* stream);
int focus_orvit_merge_bwd(const void* dout, const float* scale, void* dy, void* dmm, int B, int T, int HW, int O, int C,
                          int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Box layout (ORViT/utils.py:8-28 -> layout.py:28-63,98-130,205-237), closed form of SURVEY.md A4:
 *   out[n,y,x,:] = sum_o keep_o * vecs[n,o,:] * w((lin_y - y0_o)/y1_o) * w((lin_x - x0_o)/x1_o)
 * boxes [NF,O,4] fp32 cxcywh; vecs [NF,O,C]; out [NF,H*W,C].   NF = B*T frames.
 * ----------------------------------------------------------------------------------------------*/
int focus_box_layout_fwd(const void* vecs, const float* boxes, void* out, int NF, int O, int C, int H,
                         int W, int dtype, void* stream);
int focus_box_layout_bwd(const void* dout, const float* boxes, void* dvecs, int NF, int O, int C, int H,
                         int W, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Slot-attention inverted softmax + weighted mean (steve.py:76-83) for one frame t, one iteration:
 *   logits[b,n,k] = k_t[b,n,:].q[b,k,:]; attn_vis = softmax_k; a = (attn_vis+eps)/sum_n; upd = a^T v_t
 * k_t, v_t [B,N,D] with batch stride `kv_bstride` elements (frame t of [B,T,N,D] read in place);
 * q [B,K,D]; attn_vis [B,N,K] (stride attn_bstride); upd [B,K,D]; colsum [B,K] fp32 (saved).
 * K <= 32, D <= 256.  partial: fp32 scratch of focus_slot_attn_workspace_bytes().
 * ----------------------------------------------------------------------------------------------*/
size_t focus_slot_attn_workspace_bytes(int B, int N, int K, int D);
int focus_slot_attn_fwd(const void* k_t, const void* v_t, int64_t kv_bstride, const void* q, void* attn_vis,
                        int64_t attn_bstride, void* upd, float* colsum, void* partial, size_t partial_bytes,
                        int B, int N, int K, int D, float eps, int dtype, void* stream);
/* dattn_vis may be NULL (no cotangent on the visualised attention).  dk_t/dv_t written at the same
 * strides as k_t/v_t (accumulate=1: added to the existing contents).
 * wl != NULL (focus_slot_kv_grad_ok): d(k_t), d(v_t) are NOT formed here (dk_t, dv_t may be NULL); the launch writes its
 * rows of w = (attn + eps) / colsum and d(logits) to wl [B,N,32] bf16 (slots 0..15 | 16..31) for focus_slot_kv_grad. */
int focus_slot_attn_bwd(const void* k_t, const void* v_t, int64_t kv_bstride, const void* q,
                        const void* attn_vis, int64_t attn_bstride, const float* colsum, const void* upd,
                        const void* dupd,
                        const void* dattn_vis, void* dk_t, void* dv_t, int accumulate, void* dq, void* partial,
                        size_t partial_bytes, int B, int N, int K, int D, float eps, int dtype, void* wl, void* stream);
/* d(k_t), d(v_t) of one frame for all `iters` (<= 4) corrector iterations that read it (steve.py:68-83), from the wl rows
 * of their backward launches and their q / dupd [B,K,D]:  dk = sum_i dlogits_i . q_i,  dv = sum_i w_i . dupd_i  (two MFMA
 * products with the iterations stacked along the reduction).  bf16, K <= 16, D in {64,128,192,256}.  dk_t / dv_t rows are
 * kv_ld elements apart (>= D): with dv_t = dk_t + D and kv_ld = 2 D the two gradients form one [B,N,2D] matrix [dk | dv],
 * which lets the projections' backward run as one product each (d(input) = [dk|dv].[Wk;Wv], d[Wk;Wv] = [dk|dv]^T.x). */
/* Which kernel focus_slot_attn_fwd (backward == 0) or focus_slot_attn_bwd (backward != 0) launches for these arguments:
 * the entry points take their decision from the same host function, nothing is launched here (no GPU needed).  For the
 * forward pass dk_t, dv_t and wl as NULL.  Returns a negative status where the entry point would refuse (FOCUS_ERR_SHAPE,
 * FOCUS_ERR_ALIGN), else   kernel | full << 8 | p0 << 16 | p1 << 24   with kernel one of focus_slot_kernel, full = 1 for
 * the FULL instantiation (every row of every workgroup exists: hand-issued loads), p0 = KS (= D / 32) of the MFMA kernels
 * or KP (slots padded to 4, 8, 16, 32) of the generic ones, p1 = DV (= ceil(D / 64)) of the generic ones, else 0. */
enum focus_slot_kernel {
    FOCUS_SLOT_KERNEL_FWD_MFMA = 1,      /* slot_fwd_mfma_kernel<KS, FULL>            */
    FOCUS_SLOT_KERNEL_FWD_GENERIC = 2,   /* slot_fwd_kernel<T, KP, DV>                */
    FOCUS_SLOT_KERNEL_BWD_DEFER = 3,     /* slot_bwd_defer_kernel<KS, FULL, HAS_DA>   */
    FOCUS_SLOT_KERNEL_BWD_MFMA = 4,      /* slot_bwd_mfma_kernel<KS>                  */
    FOCUS_SLOT_KERNEL_BWD_GENERIC = 5    /* slot_bwd_kernel<T, KP, DV>                */
};
int focus_slot_attn_route(int backward, const void* k_t, const void* v_t, int64_t kv_bstride, const void* q,
                          const void* dk_t, const void* dv_t, const void* wl, int N, int K, int D, int dtype);
int focus_slot_kv_grad_ok(int K, int D, int dtype, int iters);
int focus_slot_kv_grad(const void* wl0, const void* wl1, const void* wl2, const void* wl3, const void* q0, const void* q1,
                       const void* q2, const void* q3, const void* du0, const void* du1, const void* du2, const void* du3,
                       int iters, void* dk_t, void* dv_t, int64_t kv_bstride, int64_t kv_ld, int B, int N, int K, int D,
                       int dtype, void* stream);

/* Multi-head attention over a handful of tokens (STEVE's slot predictor, transformer.py:4-49: K = 11 slots, 4 heads of 48),
 * one launch each way: q [B,N,heads*d], k, v [B,M,heads*d] with rows ldq / ldk / ldv elements apart and no gap between
 * clips (ld = heads*d: dense; the three may be the column blocks of one [B*N, 3*heads*d] projection output); att
 * [B,heads,N,M] = softmax_rows(scale q k^T) is stored for the backward; out, dout [B,N,heads*d] dense = att v.  dq, dk, dv
 * are written at the strides of q, k, v.  N, M <= 16, d <= 64 (focus_small_attn_ok); no mask, no dropout. */
int focus_small_attn_ok(int N, int M, int d);
int focus_small_attn_fwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, void* att,
                         void* out, int B, int heads, int N, int M, int d, float scale, int dtype, void* stream);
int focus_small_attn_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldk, int64_t ldv, const void* att,
                         const void* dout, void* dq, void* dk, void* dv, int B, int heads, int N, int M, int d, float scale,
                         int dtype, void* stream);

/* nn.GRUCell gate math (STEVE/utils.py:107-118): gi, gh [R,3D] gate pre-activations, h [R,D] -> hn.
 * b_ih, b_hh (fp32 [3D]; both or neither): with them gi / gh arrive WITHOUT bias (the cell's two Linear products run as one
 * batched bias-free launch), the kernel adds the biases and writes the biased values back into gi / gh -- what the
 * backward reads.  NULL: gi / gh already carry their biases and are only read. */
int focus_gru_gates_fwd(void* gi, void* gh, const void* h, void* hn, const float* b_ih, const float* b_hh, int R, int D,
                        int dtype, void* stream);
/* dh = the direct part dhn * z.  zero_out (may be NULL): an [R,D] buffer cleared by the same launch -- with dh it forms the
 * [2,R,D] residual operand of the batched product [d(input) | d(h)] = [dgi | dgh] . [W_ih | W_hh] + [0 | dh]. */
int focus_gru_gates_bwd(const void* gi, const void* gh, const void* h, const void* dhn, void* dgi, void* dgh,
                        void* dh, void* zero_out, int R, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Patch embedding as GEMM (stem_helper.py:317-320): im2col of x [B,Cin,T,H,W] fp32 (loader output)
 * for a kernel == stride patch (kt,kh,kw) -> cols [B*T'*H'*W', Cin*kt*kh*kw] in `dtype`,
 * rows in (t,h,w) token order, columns in Conv3d weight order (c,dt,dh,dw).
 * ----------------------------------------------------------------------------------------------*/
int focus_im2col_patches(const float* x, void* cols, int B, int Cin, int T, int H, int W, int kt, int kh,
                         int kw, int dtype, void* stream);

/* tokens[b,0,:] = cls + pos[0]; tokens[b,1+t*P+p,:] = patch[b,t*P+p,:] + pos[1+p] + temp[t]
 * (video_model_builder.py:1281-1320). cls [C], pos [1+P,C], temp [T,C] fp32. */
int focus_embed_assemble(const void* patch, const float* cls, const float* pos, const float* temp,
                         void* tokens, int B, int T, int P, int C, int dtype, void* stream);

/* Label-smoothing cross entropy (losses.py:53-59): loss_rows [R] fp32, dlogits [R,Ncls] fp32
 * (= d mean-loss / d logits).  logits fp32. */
int focus_xent_ls(const float* logits, const int64_t* target, float* loss_rows, float* dlogits, int R,
                  int Ncls, float smoothing, void* stream);

/* dst[c, r] = src[r, c] for src [R, Cc] with row stride src_ld; dst has row stride dst_ld >= R and
 * columns R..dst_ld-1 are zero-filled (so a transposed operand can feed the K-contiguous MFMA GEMM).
 * src may be fp32 or bf16 (src_dtype); dst is `dst_dtype`. Batched over `batch` with the given strides. */
int focus_transpose_pad(const void* src, int src_dtype, int64_t src_ld, int64_t src_bstride, void* dst,
                        int dst_dtype, int64_t dst_ld, int64_t dst_bstride, int R, int Cc, int batch,
                        void* stream);

/* bf16 working copies of fp32 master weights, all tensors of a model in ONE launch (what autocast does per use in
 * the reference, train_net.py:84 `torch.cuda.amp.autocast`): for every item, dst[r,c] = bf16(src[r,c]) (row-major,
 * optional) and dstT[c,r] = bf16(src[r,c]) (the K-contiguous operand of the dX GEMM, optional).
 * `items` is a DEVICE array of n_items focus_shadow_item; rows % 4 == 0 and cols % 4 == 0, 16-byte aligned src. */
typedef struct focus_shadow_item {
    const float* src; void* dst; void* dstT;
    int32_t rows, cols;
} focus_shadow_item;
int focus_shadow_refresh(const focus_shadow_item* items, int n_items, int max_rows, int max_cols, void* stream);

/* The optimizer step of train_net.py:108-120 for ALL parameters of a model in two launches (optim.hip): global gradient
 * norm (clip_grad_norm_, train_net.py:112-117; max_norm <= 0: no clipping), AdamW update (torch.optim.AdamW as built by
 * optimizer.py:137-145: decoupled weight decay, bias correction, no amsgrad) of the fp32 masters and moments, and the bf16
 * working copies of the updated weights (dst row-major, dstT transposed; either may be NULL).
 * `items`: DEVICE array; `grads`: DEVICE array of the n_items fp32 gradient pointers (kept apart from `items`: they are
 * the only pointers that change from step to step); unit0 = first work unit of the item (prefix sum of focus_adamw_units over the items);
 * tile_mode 1 needs rows % 4 == 0, cols % 4 == 0 and 16-byte aligned tensors (dstT only in tile mode).
 * `groups`: DEVICE [n_groups][2] = (lr, weight_decay).  `steps`: DEVICE [n_items] fp32 step counters, incremented here.
 * `total_norm`: DEVICE scalar receiving the gradient norm before clipping, or NULL.
 * write_clipped_grads: g *= clip coefficient is stored back (what clip_grad_norm_ leaves in .grad). */
typedef struct focus_adamw_item {
    float* p; float* m; float* v; void* dst; void* dstT;
    int32_t rows, cols, group, unit0, tile_mode, pad_;
} focus_adamw_item;
int focus_adamw_units(int rows, int cols, int tile_mode);
size_t focus_adamw_workspace_bytes(void);
int focus_adamw_step(const focus_adamw_item* items, float* const* grads, int n_items, int n_units, const float* groups, float* steps,
                     void* workspace, size_t workspace_bytes, float* total_norm, double beta1, double beta2, float eps,
                     float max_norm, int write_clipped_grads, void* stream);

/* The same two launches for the three update rules of the training loops (train_net.py:108-120, steve_train_net.py:116-126):
 * focus_adamw_step is this entry with mode FOCUS_OPTIM_ADAMW.  Items, gradient pointers, group table, step counters,
 * workspace and the bf16 copies are those of focus_adamw_step.  Per element, in fp32 (coef = the norm-clip coefficient, 1
 * without clipping; 1 - beta, bc1 = 1 - beta1^step and bc2 = 1 - beta2^step are formed in double):
 *   ADAMW  torch.optim.AdamW:  g = coef*g;  p -= lr*wd*p;  m += (1-b1)*(g-m);  v = b2*v + (1-b2)*g*g;
 *          p -= (lr/bc1) * (m / (sqrt(v)*(1/sqrt(bc2)) + eps))
 *   ADAM   torch.optim.Adam without amsgrad (coupled decay):  g = coef*g;  if wd: g += wd*p;  then m, v and p as above
 *          without the decoupled decay
 *   SGD    torch.optim.SGD:  g = coef*g;  if wd: g += wd*p;  with momentum > 0 and a buffer (item.m):
 *          buf = g on the buffer's FIRST use (no dampening, as torch does), buf = momentum*buf + (1-dampening)*g afterwards;
 *          g = g + momentum*buf with nesterov, else g = buf;  then p -= lr*g.
 *          item.v is not read; with momentum == 0 item.m is not read either (both may be NULL).
 * First use is a property of the buffer, not of the global step: steps[i] counts the uses of item i's buffer, the call
 * increments it, and the use that takes it to 1 is the first.  The caller starts a fresh buffer's counter at 0 (whenever
 * its first gradient arrives) and the counter of a buffer that comes from a checkpoint at >= 1.  For ADAM / ADAMW steps[i]
 * is the `step` of the bias corrections.
 * clip_value > 0: g is clamped to +-clip_value before anything else (clip_grad_value_, SOLVER.CLIP_GRAD_VAL); it excludes
 * max_norm > 0.  write_clipped_grads stores the clamped / scaled g back (scaled: only when coef < 1).  `total_norm` always
 * receives the norm of the gradients as they arrived.
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (items, grads, groups,
 * steps, workspace or hyper is NULL); FOCUS_ERR_SHAPE (an unknown mode; max_norm > 0 together with clip_value > 0; SGD
 * with nesterov and momentum <= 0 or dampening != 0); FOCUS_OK without a launch for n_items <= 0 or n_units <= 0;
 * FOCUS_ERR_WORKSPACE (fewer than focus_adamw_workspace_bytes()). */
enum focus_optim_mode { FOCUS_OPTIM_ADAMW = 0, FOCUS_OPTIM_ADAM = 1, FOCUS_OPTIM_SGD = 2 };
typedef struct focus_optim_hyper {
    double beta1, beta2;            /* ADAM, ADAMW */
    double momentum, dampening;     /* SGD */
    float eps, max_norm, clip_value;
    int32_t nesterov, write_clipped_grads, pad_;
} focus_optim_hyper;
int focus_optim_step(int mode, const focus_adamw_item* items, float* const* grads, int n_items, int n_units, const float* groups,
                     float* steps, void* workspace, size_t workspace_bytes, float* total_norm, const focus_optim_hyper* hyper,
                     void* stream);

/* OCP FP8 E4M3 working copies of fp32 master weights with one scale per tensor (BASELINE configs[4]; the reference's
 * EK_ORVIT_MF_HR.yaml trains fp16-autocast: these replace autocast's per-use fp16 weight casts, train_net.py:84):
 * scale = amax|w| / 448, dst[r,c] = e4m3(w[r,c] / scale) (row-major, optional), dstT[c,r] = the same code transposed
 * (the K-contiguous B operand of the dX GEMM, optional), *scale = the fp32 scale (1 for an all-zero tensor).
 * `items`: DEVICE array; rows % 4 == 0, cols % 4 == 0, 16-byte aligned src.  amax_scratch: n_items x 4 bytes. */
typedef struct focus_fp8_item {
    const float* src; void* dst; void* dstT; float* scale;
    int32_t rows, cols;
} focus_fp8_item;
int focus_fp8_refresh(const focus_fp8_item* items, int n_items, int max_rows, int max_cols, void* amax_scratch, void* stream);

/* Weight and bias gradients of up to 8 nn.Linear layers in ONE launch (gemm_tn_group.hip; autograd of attention.py:506,
 * 536,555 and common.py:26-34 inside one block): dw_p[N,K] = dy_p[M,N]^T . x_p[M,K] (fp32, dense), db_p[N] = column sums
 * of dy_p (stored in a fixed order, no atomics: bitwise reproducible; NULL = no bias).  bf16 operands, row strides ld_dy / ld_x in elements;
 * N, K, strides multiples of 8; 16-byte aligned pointers.  `items` is a HOST array. */
typedef struct focus_wgrad_item {
    const void* dy; const void* x; float* dw; float* db;
    int64_t ld_dy, ld_x;
    int32_t M, N, K, pad_;
} focus_wgrad_item;
int focus_linear_wgrad_group_units(const focus_wgrad_item* items, int n_items);
/* The launch's unit list (n_units x 8 bytes, HOST memory): a function of the (N, K) sequence only; the caller keeps a DEVICE
 * copy per shape signature and hands it to focus_linear_wgrad_group. */
int focus_linear_wgrad_group_plan(const focus_wgrad_item* items, int n_items, void* host_units, size_t bytes);
int focus_linear_wgrad_group(const focus_wgrad_item* items, int n_items, const void* dev_units, void* stream);

/* The per-iteration tail of the STEVE slot update in one launch (slot_tail.hip; steve.py:72-75,85-93, STEVE/utils.py:107-118):
 * [do_gru] GRU cell on (upd, h) -> hn;  [do_mlp] s = hn + W2 relu(W1 LN1(hn) + b1) + b2;  [do_q] q = Wq LN2(slots) where slots
 * is s, hn or (do_gru == 0: "q only") the input h itself.  R rows of D (= 192) channels, hidden width H (= 768); bf16
 * activations and weights ([out, in] row-major, the bf16 working copies), fp32 biases / LayerNorm parameters / statistics.
 * Every intermediate a backward needs is an output: g [2,R,3D] (gate pre-activations incl. bias), hn, y = LN1(hn) with
 * mean1 / rstd1 [R], a = relu(..) [R,H], s, sn = LN2(slots) with mean2 / rstd2, q.
 * Status (pinned by tests/test_gpu_slot_tail.py; a refused call writes nothing): args NULL is FOCUS_ERR_NULL; R <= 0 returns
 * FOCUS_OK without a launch, whatever else the arguments hold; D, H other than 192, 768 and do_mlp without do_gru (the MLP
 * normalises h' and adds to it) are FOCUS_ERR_SHAPE; a NULL pointer of a stage that is switched on (h always) is
 * FOCUS_ERR_NULL.  The pointers of a stage that is switched off are not looked at and its outputs are not written.  Rows are
 * dense (stride D, H, 3D; plane 1 of g starts at row R); nothing is read or written past row R - 1 of any tensor.
 * FOCUS_SLOT_TAIL_STAGED (read per call; default 1) selects four right-sized launches (1) or one launch (0): same stored
 * values, LayerNorm sums associated differently. */
typedef struct focus_slot_tail_args {
    int32_t R, D, H, do_gru, do_mlp, do_q;
    float ln1_eps, ln2_eps;
    const void* upd; const void* h;
    const void* w_ih; const void* w_hh; const float* b_ih; const float* b_hh;
    const float* ln1_g; const float* ln1_b; const void* w1; const float* b1; const void* w2; const float* b2;
    const float* ln2_g; const float* ln2_b; const void* wq;
    void* g; void* hn; void* y; float* mean1; float* rstd1; void* a; void* s;
    void* sn; float* mean2; float* rstd2; void* q;
} focus_slot_tail_args;
int focus_slot_tail_ok(int D, int H, int dtype);
int focus_slot_tail_fwd(const focus_slot_tail_args* args, void* stream);
/* The same chain backwards in one launch (autograd of steve.py:84-93 / utils.py:107-118 per iteration), against the TRANSPOSED
 * bf16 weight copies ([in][out]).  Inputs: dout (gradient of the slots; may be NULL = 0), dq (with do_q), the forward's saved
 * tensors (cur = the slots LayerNorm_slots normalised: s, or hn without the MLP, or h without the GRU).  Outputs: dupd, dh
 * [R,D]; the dY rows the weight gradients are later formed from: ds [R,D] (fc2; also with do_q alone), dz [R,H] (fc1), dg
 * [2,R,3D] (W_ih, W_hh) (dq itself is Wq's); LayerNorm parameter partials part1 / part2 [2][focus_slot_tail_bwd_blocks(R)][D]
 * fp32 ([0] = d gamma, [1] = d beta; sum over the blocks; a block is 16 consecutive rows).
 * Which outputs a call writes: dh always; dupd, dg with do_gru; dz, part1, ds with do_mlp (without do_q: ds = dout, zeros for
 * NULL); part2, ds with do_q -- except the staged form without do_gru, which writes dh only (dh = ds there; the one launch
 * writes both); with neither do_q nor do_mlp ds is not looked at.  Everything else keeps its contents.
 * Status (pinned by tests/test_gpu_slot_tail.py; a refused call writes nothing): args NULL is FOCUS_ERR_NULL; R <= 0 returns
 * FOCUS_OK without a launch; D, H other than 192, 768 and do_mlp without do_gru are FOCUS_ERR_SHAPE; dh NULL, or a NULL input
 * or output of a stage that is switched on, is FOCUS_ERR_NULL (do_q: dq, cur, mean2, rstd2, ln2_g, wq_t, ds, part2; do_mlp: a,
 * hn, mean1, rstd1, ln1_g, w1_t, w2_t, ds, dz, part1; do_gru: g, h, w_ih_t, w_hh_t, dg, dupd).  The staged form
 * (FOCUS_SLOT_TAIL_STAGED unset or non-zero) further needs its scratch, ws_dsn with do_q, ws_dy1 with do_mlp, ws_res with
 * do_gru (FOCUS_ERR_WORKSPACE), and has nothing to launch with neither do_gru nor do_q (FOCUS_ERR_SHAPE; the one launch
 * copies dout to dh). */
typedef struct focus_slot_tail_bwd_args {
    int32_t R, D, H, do_gru, do_mlp, do_q;
    const void* dout; const void* dq;
    const void* h; const void* g; const void* hn; const void* a; const void* cur;
    const float* mean1; const float* rstd1; const float* mean2; const float* rstd2;
    const float* ln1_g; const float* ln2_g;
    const void* w_ih_t; const void* w_hh_t; const void* w1_t; const void* w2_t; const void* wq_t;
    void* dupd; void* dh; void* ds; void* dz; void* dg; float* part1; float* part2;
    void* ws_dsn; void* ws_dy1; void* ws_res;     /* [R, D] bf16 scratch between the launches of the staged form (do_q / do_mlp / do_gru) */
} focus_slot_tail_bwd_args;
int focus_slot_tail_bwd_blocks(int R);
int focus_slot_tail_bwd(const focus_slot_tail_bwd_args* args, void* stream);

/* Multi-head attention without the [Nq, Nk] probabilities in memory (flash_attn.hip) -- the STEVE decoder's causal
 * self-attention over the image tokens of a frame: STEVE/transformer.py:23-49 (MultiHeadAttention.forward: scale, mask,
 * softmax, dropout on the probabilities, product with v) with the upper-triangular mask of :131-132 / :149-151, and its autograd.
 *   out[b, n, h*d:(h+1)*d] = dropout(softmax_k(scale * q.k + causal mask)) v        lse[b, h, n] = log sum_k exp(scale * q.k)
 * q / k / v / out / dout / dq / dk / dv: bf16 rows of `heads * d` channels, row strides ld*, batch strides bs* (elements; the
 * three inputs may be column blocks of one projection output).  d in {32, 48, 64}; causal needs Nq == Nk.
 * drop_thr = round(p * 65536) (0: no dropout): element (b*heads + h, query, key) is kept iff the 16-bit half (key & 1) of
 * lowbias32(seed[0] ^ (bh * 0x9E3779B1) ^ (query * 0x85EBCA77) ^ ((key >> 1) * 0xC2B2AE3D)) is >= drop_thr, kept values are
 * scaled by 65536 / (65536 - drop_thr); `seed` is read on the device, so a draw can be captured in a graph.
 * bwd: delta [B, heads, Nq] fp32 is scratch (written by the dQ kernel, read by the dK/dV kernel); dq, dk, dv fully written. */
typedef struct focus_flash_args {
    const void* q; const void* k; const void* v; void* out; float* lse;
    const void* dout; float* delta; void* dq; void* dk; void* dv;
    const uint32_t* seed;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int64_t bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;
    int32_t B, heads, Nq, Nk, d, dtype, causal;
    uint32_t drop_thr;
    float scale;
    int32_t pad_;
} focus_flash_args;
int focus_flash_attn_ok(int Nq, int Nk, int d, int dtype, int causal);
int focus_flash_attn_fwd(const focus_flash_args* args, void* stream);
int focus_flash_attn_bwd(const focus_flash_args* args, void* stream);

/* One step of greedy autoregressive decoding (decode_attn.hip; steve.py:359-381, STEVE.decode): attention of ONE new query
 * row per sequence over a key/value cache, and the arg-max / embedding that ends the step.
 * focus_decode_attn: q, out [B, heads*d] rows ldq / ldo elements apart; k_cache, v_cache [B, Lmax, heads*d] with row stride
 * ldc and batch stride bsc.  `len` (1 <= len <= Lmax) = number of valid keys AFTER the call.
 *   k_new, v_new [B, heads*d] rows ldn apart (q | k_new | v_new may be the column blocks of one projection output): row
 *   len-1 of both caches is first written from them bit for bit, then out = softmax(scale q K^T) V per head over rows
 *   0 .. len-1.  Both NULL: the caches are only read (cross-attention over the projected slots, len = their number).
 * Rows >= len of the caches are neither read into the result nor written; nothing else is written.
 * d % 8 == 0, 8 <= d <= 64, fp32 or bf16 storage with fp32 accumulation (focus_decode_attn_ok).  Every pointer 16-byte
 * aligned, every stride >= heads*d and a multiple of 16 bytes (FOCUS_ERR_ALIGN otherwise). */
int focus_decode_attn_ok(int Lmax, int d, int dtype);
int focus_decode_attn(const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ldn, void* k_cache,
                      void* v_cache, int64_t ldc, int64_t bsc, void* out, int64_t ldo, int B, int heads, int d, int len,
                      int Lmax, float scale, int dtype, void* stream);
/* tok[b * tok_stride] = argmax_v logits[b, v] (lowest index on ties; a NaN counts as the largest value, as in
 * torch.argmax) and x_next[b, :] = dict[tok, :] + pe_row rounded to `dtype`: the next step's input row.  logits [B, V] and
 * x_next [B, D] in `dtype` with row strides ldl / ldx; dict [V, D] and pe_row [D] fp32 dense. */
int focus_greedy_next(const void* logits, int64_t ldl, const float* dict, const float* pe_row, int64_t* tok,
                      int64_t tok_stride, void* x_next, int64_t ldx, int B, int V, int D, int dtype, void* stream);

/* Both consumers of g = d(loss)/d(u) of the re-associated temporal step in one pass over g (traj_time2_gw.hip; autograd of
 * attention.py:536-549): dq2[r, h*d+dd] = sum_c g[h,r,c] Wk[h*d+dd, c] and dWk[h*d+dd, c] = sum_r q2[r, h*d+dd] g[h,r,c].
 * g [heads][R][C] bf16, q2 / dq2 [R][C] bf16, wk = the bf16 rows of Wk (row stride wk_ld), dwk [C][C] fp32 dense.
 * bf16, d = 64, C = 768, R % 32 == 0 (focus_traj_time2_gw_ok); ws: focus_traj_time2_gw_workspace_bytes.
 * Status, in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE
 * (not focus_traj_time2_gw_ok, wk_ld % 8 != 0); FOCUS_ERR_ALIGN (g, q2, wk or dwk not 16-byte aligned);
 * FOCUS_ERR_WORKSPACE (ws_bytes too small). */
int focus_traj_time2_gw_ok(int R, int heads, int d, int dtype);
size_t focus_traj_time2_gw_workspace_bytes(int R, int heads, int d);
int focus_traj_time2_gw(const void* g, const void* q2, const void* wk, int64_t wk_ld, void* dq2, float* dwk, void* ws,
                        size_t ws_bytes, int R, int heads, int d, int dtype, void* stream);

/* Row passes over the [frames * tokens, vocabulary] tensors of STEVE.forward (gumbel.hip); one workgroup per row, the row in
 * registers: V % 8 == 0, 8 <= V <= 8192, R < 2^31, dtype fp32 or bf16 (focus_rows_ok).
 *
 * focus_gumbel_fwd (steve.py:262-271 with utils.py:47-61): logp = log_softmax(x);  z = softmax((logp + G_soft) / tau), or the
 * straight-through value (one_hot(argmax z) - z) + z when `hard`;  target[r] = argmax(logp + G_hard) -- the only use the
 * reference makes of its second, hard sample (target may be NULL).  G = -log(E + tiny), E ~ Exp(1): e_soft / e_hard [R, V]
 * fp32 are the draws (the reference's torch.empty_like(logits).exponential_()), or both NULL and the draws are generated in
 * the kernel from `seed` (4 x uint32 on the device: soft stream, hard stream), which the backward regenerates.
 * x, dx [R, V] `dtype`; z, dz [R, V] `dtype_z` (= dtype, or bf16 under fp32 logits: a bf16 decoder behind an fp32 encoder);
 * stats [R, 4] fp32 (row max, log-sum, and the same of the tempered logits) for the backward.
 * focus_gumbel_bwd: dx = d(loss)/d(x) from dz = d(loss)/d(z) (gradient of the soft sample in both modes). */
int focus_rows_ok(int64_t R, int V, int dtype);
int focus_gumbel_fwd(const void* x, const float* e_soft, const float* e_hard, const void* seed, void* z, int64_t* target,
                     float* stats, int64_t R, int V, float tau, int hard, int dtype, int dtype_z, void* stream);
int focus_gumbel_bwd(const void* x, const float* e_soft, const void* seed, const float* stats, const void* dz, void* dx,
                     int64_t R, int V, float tau, int dtype, int dtype_z, void* stream);

/* Label-smoothing cross entropy (losses.py:53-59; steve.py:303-306 with smoothing 0) on fp32 or bf16 logits [R, V]:
 * loss_rows [R] and the row log-sum-exp lse [R] fp32; the backward rebuilds softmax from lse and writes
 * dlogits = ((softmax - (1 - smoothing) onehot - smoothing / V) / R) * g[0] in `dtype` (g: device scalar, fp32). */
int focus_xent_rows_fwd(const void* logits, const int64_t* target, float* loss_rows, float* lse, int64_t R, int V,
                        float smoothing, int dtype, void* stream);
int focus_xent_rows_bwd(const void* logits, const int64_t* target, const float* lse, const float* g, void* dlogits,
                        int64_t R, int V, float smoothing, int dtype, void* stream);

/* out[i] = (res ? res[i] : 0) + keep(i) * y[i] * 65536 / (65536 - thr): a residual branch that ends in nn.Dropout
 * (transformer.py:45-47, :147-163) in one pass.  keep(i) = 16 hashed bits of (seed, i) >= thr, thr = round(p * 65536);
 * seed: 2 x uint32 on the device.  The branch's backward is the same call on the incoming gradient with res = NULL.
 * n % 8 == 0, 16-byte aligned pointers, fp32 or bf16. */
int focus_dropout_add(const void* y, const void* res, const void* seed, int thr, void* out, int64_t n, int dtype,
                      void* stream);

/* xdiag[b,s,:] = xt[b,s,s/P,:] (attention.py:533-535) and its adjoint dxt[b,s,s/P,:] += dxdiag[b,s,:]. */
int focus_diag_gather(const void* xt, void* xdiag, int B, int S, int F, int C, int dtype, void* stream);
int focus_diag_scatter_add(const void* dxdiag, void* dxt, int B, int S, int F, int C, int dtype, void* stream);

/* out[b, i] = (x ? x[b, i] : 0) + s[b] * y[b, i]   for b < B, i < per  (per % 8 == 0).
 * Stochastic depth on a residual branch in one pass (common.py:46-60: x + drop_path(y)) and its adjoint (dy = s * dout
 * with x == NULL).  keep == 0: s = scale.  keep > 0: scale holds the U[0,1) draws and s[b] = floor(keep + scale[b]) / keep
 * (the reference's mask / keep_prob, formed in the kernel instead of by three elementwise launches). */
int focus_scale_add(const void* x, const void* y, const float* scale, float keep, void* out, int B, int64_t per,
                    int dtype, void* stream);

/* dtype conversion (weights shadow copies, gradient casts): n elements. */
int focus_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d and MaxPool2d(3, 2, 1) over channels-last feature maps (batchnorm.hip; the ResNet-18 trunk of STEVE,
 * steve.py:175-202).  Every tensor is a row matrix [R, C], R = N*H*W, dense with row stride C; C % 8 == 0, 8 <= C <= 256;
 * activations (x, y, residual, dy, dx, dres) in `dtype` (fp32 or bf16), statistics and affine parameters fp32.  A thread
 * owns 8 consecutive channels (16-byte accesses); reductions over the rows are two-stage and in a fixed order (no atomics):
 * the same inputs give the same bits.
 *
 * focus_bn_blocks(R): the number of row blocks of the reductions, >= 1 (host only).  focus_bn_workspace_bytes(R, C): the size
 * of the caller-owned `workspace` of focus_bn_stats and focus_bn_bwd (host only; 0 for a C the kernels refuse).
 *
 * focus_bn_stats (training mode): mean[C] and rstd[C] = 1 / sqrt(var + eps), var the BIASED variance over the R rows.  Stage 1
 *   leaves per-block (count, mean, M2) partials in the workspace (Welford: never E[x^2] - E[x]^2), stage 2 merges them
 *   pairwise (Chan).  running_mean / running_var (both or neither; may be NULL) are updated in place:
 *   r = (1 - momentum) r + momentum s, s the batch mean / the UNBIASED variance M2 / (R - 1), as nn.BatchNorm2d does.
 *   R < 2 is FOCUS_ERR_SHAPE (torch raises there too).
 * focus_bn_apply: y = act(gamma (x - mean) rstd + beta [+ residual]), act = ReLU (relu != 0) or the identity.  Eval mode is
 *   the same call with mean / rstd formed from the running buffers.  residual may be NULL.
 * focus_bn_bwd: g = dy (y > 0) when relu (the mask is read from the stored output y; y may be NULL otherwise), else g = dy;
 *   dbeta = sum g, dgamma = sum g x^ (x^ = (x - mean) rstd); dx = gamma rstd (g - dbeta / R - x^ dgamma / R), or with
 *   frozen != 0 (eval-mode statistics) dx = gamma rstd g; dres = g when dres is not NULL (the forward had a residual).
 *
 * focus_maxpool_fwd: x [N, H, W, C] -> y [N, OH, OW, C], OH = (H - 1) / 2 + 1, and idx [N, OH, OW, C] int8 = kh * 3 + kw of the
 *   selected window position: the first maximum in row-major window order, padded positions skipped, a NaN counting as a
 *   maximum (ATen's rule).  focus_maxpool_bwd: dx[n, h, w, c] = sum of dy over the <= 4 windows that cover (h, w) and whose
 *   idx points at it (a gather: every element of dx is written once).
 *
 * Status, judged in this order before any launch: FOCUS_ERR_NULL (a required pointer is NULL; running_mean without
 * running_var or the reverse; y NULL with relu in the backward), FOCUS_ERR_SHAPE (C % 8, C < 8, C > 256, R < 0, R < 2 for
 * the statistics, N < 0, H < 1, W < 1, N*H*W >= 2^31 for the pool), FOCUS_ERR_DTYPE (neither fp32 nor bf16), FOCUS_ERR_ALIGN
 * (any pointer not 16-byte aligned).  R == 0 / N == 0 is FOCUS_OK without a launch (focus_bn_bwd zero-fills dgamma and
 * dbeta), except for focus_bn_stats.
 * ----------------------------------------------------------------------------------------------*/
int focus_bn_blocks(int64_t R);
size_t focus_bn_workspace_bytes(int64_t R, int C);
int focus_bn_stats(const void* x, float* mean, float* rstd, float* running_mean, float* running_var, void* workspace,
                   int64_t R, int C, float eps, float momentum, int dtype, void* stream);
int focus_bn_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                   const void* residual, void* y, int64_t R, int C, int relu, int dtype, void* stream);
int focus_bn_bwd(const void* dy, const void* x, const void* y, const float* mean, const float* rstd, const float* gamma,
                 void* dx, void* dres, float* dgamma, float* dbeta, void* workspace, int64_t R, int C, int relu,
                 int frozen, int dtype, void* stream);
int focus_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int dtype, void* stream);
int focus_maxpool_bwd(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clip sampling (clip_sample.hip): decoded uint8 clips -> model inputs in one launch.  The reference's three spatial
 * sampling modes (datasets/utils.py:111-188: short-side jitter + random crop, random resized crop, the test views 0/1/2),
 * its tensor_normalize (utils.py:319-336) and the channel reversal of pack_pathway_output (utils.py:86-87) are one
 * operation: the source rectangle (sy0, sx0, sh, sw) of a frame is virtually resized to (rh, rw) with bilinear
 * interpolation, align_corners=False, and the out_h x out_w window at offset (oy0, ox0) of that virtual image is
 * written, mirrored in x when flip != 0.  For output pixel (y, x) of clip b, frame t, channel c:
 *     xo = flip ? out_w-1-x : x
 *     sy = max((y  + oy0 + 0.5f) * ((float)sh / rh) - 0.5f, 0);  y0 = min((int)sy, sh-1);  y1 = min(y0+1, sh-1);  ly = sy - y0
 *     sx = max((xo + ox0 + 0.5f) * ((float)sw / rw) - 0.5f, 0);  x0, x1, lx likewise
 *     v  = bilinear of src[t][sy0 + y{0,1}][sx0 + x{0,1}][c'] with (1-l, l) weights,  c' = reverse ? 2-c : c
 *     out[b*sb + c*sc + t*st + y*out_w + x] = (v/255 - mean[c']) / std[c']          (fp32 arithmetic, one rounding to `dtype`)
 * mean / std are indexed by the SOURCE channel: the reference reverses the channels after it has normalised them.
 * Rows and planes of the output are dense (row stride out_w); sb, sc, st are the clip, channel and frame strides in
 * elements, so one kernel writes [B,C,T,S,S] (Motionformer) and [B,T,C,S,S] (STEVE; mean 0, std 1 gives its [0,1] input).
 *
 * `items`: DEVICE array of n_clips descriptors owned by the caller; the clips of one launch may differ in everything a
 * descriptor holds.  src is [T][H][W][3] uint8 with row_stride / frame_stride in BYTES (no alignment requirement: rows are
 * read byte-wise).  `mean`, `std`: HOST pointers to 3 floats each, read before the call returns; std[c] != 0.  `out` has no
 * alignment requirement beyond its element size (16-byte stores are used where the address allows them).  The same
 * arguments give the same bits (no atomics, no workspace).
 *
 * The descriptors live on the device, so this entry point cannot judge them: the caller guarantees 0 <= sy0, sy0 + sh <= H,
 * 0 <= sx0, sx0 + sw <= W, sh, sw, rh, rw >= 1 and 0 <= oy0, oy0 + out_h <= rh, 0 <= ox0, ox0 + out_w <= rw
 * (focus_amd.ops.clip_sample raises ValueError otherwise).  The kernel clamps the rectangle to the frame before it reads,
 * and skips a clip whose rectangle or virtual size is empty, so a bad descriptor cannot read outside [0,H) x [0,W).
 *
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (items, out, mean or std is
 * NULL); FOCUS_OK without a launch for n_clips <= 0 or T <= 0; FOCUS_ERR_SHAPE (out_h <= 0, out_w <= 0, T or n_clips above
 * 65535); FOCUS_ERR_DTYPE (neither FOCUS_F32 nor FOCUS_BF16).
 * ----------------------------------------------------------------------------------------------*/
typedef struct focus_clip_item {
    const uint8_t* src;
    int64_t row_stride, frame_stride;
    int32_t H, W, sy0, sx0, sh, sw, rh, rw, oy0, ox0, flip, pad_;
} focus_clip_item;
int focus_clip_sample(const focus_clip_item* items, int n_clips, int T, int out_h, int out_w, void* out,
                      int64_t sb, int64_t sc, int64_t st, const float* mean, const float* std, int reverse, int dtype,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clip sampling with a colour stage (clip_color.hip): the AVA front end (ava_dataset.py:255-365 with
 * AVA.IMG_PROC_BACKEND "pytorch"; transform.py:297-517: color_jitter, lighting_jitter, color_normalization).  Descriptors,
 * taps, output addressing (sb, sc, st) and dtypes are focus_clip_sample's.  Between /255 and the normalisation every clip
 * runs the ops of its focus_clip_color record, in the record's order; per pixel, x[c'] by SOURCE channel c':
 *     x[c'] = v[c'] / 255                                                  (v: focus_clip_sample's bilinear value)
 *     for i < n_ops:   a = alpha[i]
 *         FOCUS_COLOR_BRIGHTNESS   x[c'] = x[c'] * a
 *         FOCUS_COLOR_SATURATION   x[c'] = x[c'] * a + g * (1 - a),    g = sum_c' gray_w[c'] * x[c']  of this pixel, now
 *         FOCUS_COLOR_CONTRAST     x[c'] = x[c'] * a + m_t * (1 - a),  m_t = frame_mean[b*T + t]
 *     x[c'] += shift[c']                                                   (the PCA lighting shift; 0 = none)
 *     out[b*sb + c*sc + t*st + y*out_w + x] = (x[c'] - mean[c']) / std[c'],   c' = reverse ? 2-c : c
 * m_t is the mean over the out_h x out_w output window of frame t ALONE of the grey g of the pixel as it stands when
 * contrast runs: resampled, windowed, mirrored, and after the ops listed before contrast.  Nothing is clamped.  gray_w,
 * shift, mean and std are indexed by the source channel (a BGR source: gray_w = {0.114, 0.587, 0.299}).  Every kind occurs
 * at most once in a record and alpha / shift are finite (focus_amd.ops.clip_sample_color raises ValueError otherwise; the
 * kernels read n_ops clamped to 0..3 and treat an unknown kind as saturation).
 *
 * focus_clip_gray_mean writes frame_mean[n_clips * T] (fp32): m_t for a clip whose ops contain contrast, 0 for every other
 * clip.  It is a reduction with a fixed order and no floating-point atomics (8 pixels per thread in x order, a 64-lane
 * butterfly, the block's four waves in order, one partial per block in the workspace, the partials in block order by the
 * block that arrives last -- told by an integer ticket), so the same arguments give the same bits.  The workspace is
 * caller-owned, 4-byte aligned, at least focus_clip_color_workspace_bytes(...) long (0 for an empty or refused shape),
 * needs no initialisation and holds nothing between calls.  A batch without any contrast op needs no call at all:
 * focus_clip_sample_color reads frame_mean only for clips with contrast.  focus_clip_sample_color has no workspace and no
 * atomics.  `colors`: DEVICE array of n_clips records; gray_w, mean, std: HOST pointers to 3 floats, read before return.
 *
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (any pointer; the
 * workspace too); FOCUS_OK without a launch for n_clips <= 0 or T <= 0; FOCUS_ERR_SHAPE (as focus_clip_sample);
 * focus_clip_gray_mean then FOCUS_ERR_ALIGN (frame_mean or workspace not 4-byte aligned) and FOCUS_ERR_WORKSPACE
 * (workspace_bytes too small); focus_clip_sample_color then FOCUS_ERR_DTYPE.
 * ----------------------------------------------------------------------------------------------*/
enum focus_color_op { FOCUS_COLOR_BRIGHTNESS = 0, FOCUS_COLOR_CONTRAST = 1, FOCUS_COLOR_SATURATION = 2 };
typedef struct focus_clip_color {
    int32_t n_ops;
    int32_t op[3];       /* 0..3 ops, applied in this order, each kind at most once */
    float alpha[3];      /* blend weight of op[i] */
    float shift[3];      /* added after the ops, by source channel */
} focus_clip_color;
size_t focus_clip_color_workspace_bytes(int n_clips, int T, int out_h, int out_w);
int focus_clip_gray_mean(const focus_clip_item* items, const focus_clip_color* colors, int n_clips, int T, int out_h,
                         int out_w, const float* gray_w, float* frame_mean, void* workspace, size_t workspace_bytes,
                         void* stream);
int focus_clip_sample_color(const focus_clip_item* items, const focus_clip_color* colors, const float* frame_mean,
                            int n_clips, int T, int out_h, int out_w, void* out, int64_t sb, int64_t sc, int64_t st,
                            const float* mean, const float* std, const float* gray_w, int reverse, int dtype,
                            void* stream);

/* -------------------------------------------------------------------------------------------------
 * Mixup / CutMix of a batch of clips and the soft-target loss that goes with them (mixup.hip; datasets/mixup.py:40-192 and
 * losses.py:15-36 of the reference).  Sample i of the batch is always paired with sample B-1-i (x.flip(0)).  r() below is
 * one round-to-nearest-even to the tensor's type; all arithmetic runs in fp32 and is never contracted into an fma, so the
 * results carry the bits of ATen's separately rounded mul_ / mul_ / add_.  lam and one_minus_lam are the fp32 roundings of
 * the host doubles lam and 1.0 - lam.  No workspace, no atomics: the same call gives the same bits.
 *
 * focus_mixup_blend: x [B, n_per_sample] contiguous, in place:
 *     x[i] <- r(r(x[i] lam) + r(x[B-1-i] oml)),   x[B-1-i] <- r(r(x[B-1-i] lam) + r(x[i] oml))
 *   both computed from the values loaded before either is stored; the middle sample of an odd batch pairs with itself:
 *   r(r(a lam) + r(a oml)).  16-byte accesses when x is 16-byte aligned and n_per_sample * elemsize % 16 == 0, else scalar.
 *   Status in this order: FOCUS_ERR_NULL (x); FOCUS_ERR_SHAPE (B < 1, n_per_sample < 1); FOCUS_ERR_DTYPE (neither fp32 nor
 *   bf16); FOCUS_ERR_ALIGN (x not aligned to its element size).
 *
 * focus_cutmix_paste: x [B, M, H, W] contiguous, in place: the rectangle [yl,yh) x [xl,xh) of every plane is swapped
 *   between samples i and B-1-i (x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]); the middle sample of an odd batch
 *   and every byte outside the rectangle are not touched.  Status in this order: FOCUS_ERR_NULL (x); FOCUS_ERR_SHAPE
 *   (B, M, H or W < 1, yl < 0, yh > H, yl > yh, xl < 0, xh > W, xl > xh); FOCUS_ERR_DTYPE; FOCUS_ERR_ALIGN (as above);
 *   FOCUS_OK without a launch for an empty rectangle or B == 1.
 *
 * focus_mixup_target: labels [B] int64 -> target [B,V] fp32,
 *     target[b,c] = r(r(t1 lam) + r(t2 oml)),  t1 = c == labels[b] ? on : off,  t2 = c == labels[B-1-b] ? on : off.
 *   A label outside [0,V) matches no column.  Status: FOCUS_ERR_NULL (labels, target); FOCUS_ERR_SHAPE (B < 1, V < 1).
 *
 * focus_xent_soft: logits, target [R,V] fp32 -> loss_rows [R] = lse sum(y) - sum(y x) = sum(-y log_softmax(x)) and
 *   dlogits [R,V] = (softmax(x) sum(y) - y) / R, the gradient of the mean over rows.  Targets need not sum to 1.  One
 *   256-thread workgroup per row, any V >= 1.  Status: FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE (R < 1, V < 1).
 * ----------------------------------------------------------------------------------------------*/
int focus_mixup_blend(void* x, int64_t B, int64_t n_per_sample, float lam, float one_minus_lam, int dtype, void* stream);
int focus_cutmix_paste(void* x, int64_t B, int64_t M, int H, int W, int yl, int yh, int xl, int xh, int dtype,
                       void* stream);
int focus_mixup_target(const int64_t* labels, float* target, int B, int V, float on, float off, float lam,
                       float one_minus_lam, void* stream);
int focus_xent_soft(const float* logits, const float* target, float* loss_rows, float* dlogits, int R, int V,
                    void* stream);

/* -------------------------------------------------------------------------------------------------
 * RandAugment on decoded uint8 frames (randaug.hip; datasets/rand_augment.py of the reference, which runs the ops through
 * PIL on a loader worker).  The unit of work is one frame, uint8 [H][W][3] with a row stride in BYTES, and one op; one call
 * runs one LAYER (one op slot of the policy) for every frame of a batch, each frame with its own op, size and buffers, in at
 * most two launches: a stats launch (only when need_stats != 0) and the apply launch.  A policy of n layers is n calls that
 * ping-pong between caller-owned buffers; src is never written.  The arithmetic is PIL's, bit for bit:
 *
 *   table ops   out = lut[c][in], a 256-entry table per channel built by every apply workgroup at its start.
 *               INVERT 255-v;  POSTERIZE v & ~(2^(8-iarg)-1) (iarg >= 8: identity);  SOLARIZE v < iarg ? v : 255-v;
 *               SOLARIZE_ADD v < 128 ? min(255, v+iarg) : v;  BRIGHTNESS blend(0, v, farg);
 *               AUTOCONTRAST (cutoff 0): lo / hi = first / last occupied bin of the channel's histogram; hi <= lo: identity;
 *                 else scale = 255.0/(hi-lo), offset = -lo*scale (fp64), lut = clamp((int)(v*scale + offset), 0, 255);
 *               EQUALIZE: step = (sum(h) - h[last occupied]) / 255 (integers); fewer than two occupied bins or step == 0:
 *                 identity; else lut[v] = min(255, (step/2 + sum(h[0..v-1])) / step).
 *   blend ops   blend(d, v, f) = clamp-then-truncate of  fp32(d) + f * fp32(v - d),  the product and the sum rounded
 *               separately (never an fma).  COLOR d = L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;  CONTRAST d =
 *               (int)(mean(L) + 0.5), the mean in fp64 from the stats launch;  SHARPNESS d = the 3x3 SMOOTH filter
 *               (1 1 1 / 1 5 1 / 1 1 1) / 13 in fp32, accumulated from 0.5 row by row (y+1, y, y-1), border pixels copied.
 *   affine ops  ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y are one kernel path: for output pixel (x, y)
 *               xs = coef[0]*(x+0.5) + coef[1]*(y+0.5) + coef[2],  ys = coef[3]*(x+0.5) + coef[4]*(y+0.5) + coef[5]  (fp64);
 *               the pixel is `fill` exactly when xs < 0, xs >= W, ys < 0 or ys >= H; else it is resampled at (xs-0.5, ys-0.5)
 *               with PIL's bilinear (resample 2) or bicubic (resample 3, a = -0.5) filter in fp64, neighbours clamped to the
 *               frame, truncated (bicubic: clamped first).  The host computes the coefficients: no trigonometry here.
 *   COPY        out = in (a frame whose draw left it unchanged).
 *
 * Stats: FOCUS_RANDAUG_STAT_WORDS 32-bit words per frame that asks for them (stats_off >= 0, an offset in WORDS into the
 * workspace, even): words [0,768) the histograms h[c][v], words 768-769 the 64-bit sum of L.  LDS histograms per workgroup
 * are merged with vector atomics, so the CALLER ZEROES the words of a frame before the call; integer sums are the same in
 * any order.  AUTOCONTRAST, EQUALIZE and CONTRAST need a slot (stats_off >= 0; without one the frame is copied) and
 * need_stats != 0 (with need_stats == 0 and a workspace, the slot is read as the caller left it).
 *
 * `items`: DEVICE array of n_items descriptors, owned by the caller.  This entry point cannot read it: the caller guarantees
 * valid pointers and strides, H <= max_h, W <= max_w (a larger frame is skipped), op and resample codes from the lists
 * below (an unknown op copies, an unknown resample is bilinear) and stats_off + FOCUS_RANDAUG_STAT_WORDS within the
 * workspace (a slot outside workspace_bytes is ignored and its frame copied).  focus_amd.ops.randaug_apply validates all of
 * it.  No allocation, no synchronisation, no host round trip.
 *
 * Status, in this order, before any launch: FOCUS_ERR_NULL (items; workspace when need_stats); FOCUS_OK without a launch
 * for n_items <= 0; FOCUS_ERR_SHAPE (max_h or max_w outside [1, 32768], n_items > 65535); FOCUS_ERR_ALIGN (workspace not
 * 8-byte aligned); FOCUS_ERR_WORKSPACE (need_stats and workspace_bytes < focus_randaug_workspace_bytes(1)).
 * ----------------------------------------------------------------------------------------------*/
#define FOCUS_RANDAUG_STAT_WORDS 776
enum focus_randaug_op {
    FOCUS_RA_COPY = 0, FOCUS_RA_AUTOCONTRAST = 1, FOCUS_RA_EQUALIZE = 2, FOCUS_RA_INVERT = 3, FOCUS_RA_POSTERIZE = 4,
    FOCUS_RA_SOLARIZE = 5, FOCUS_RA_SOLARIZE_ADD = 6, FOCUS_RA_BRIGHTNESS = 7, FOCUS_RA_COLOR = 8, FOCUS_RA_CONTRAST = 9,
    FOCUS_RA_SHARPNESS = 10, FOCUS_RA_ROTATE = 11, FOCUS_RA_SHEAR_X = 12, FOCUS_RA_SHEAR_Y = 13, FOCUS_RA_TRANSLATE_X = 14,
    FOCUS_RA_TRANSLATE_Y = 15
};
#define FOCUS_RA_BILINEAR 2 /* PIL's codes */
#define FOCUS_RA_BICUBIC 3
typedef struct focus_randaug_item {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_stride, dst_stride, stats_off;
    double coef[6];
    float farg;
    int32_t iarg, H, W, op, resample;
    uint8_t fill[4];
    int32_t pad_;
} focus_randaug_item;
size_t focus_randaug_workspace_bytes(int n_stats_frames);
int focus_randaug_layer(const focus_randaug_item* items, int n_items, int max_h, int max_w, int need_stats,
                        void* workspace, size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Slot masks -> segments, ORViT boxes and FG-ARI tables (slot_segments.hip): the hand-off from STEVE's slot attention
 * (steve.py:333-353 of the reference, whose masks leave the model upsampled to the frame) to meta['orvit_bboxes'] and to
 * the FG-ARI evaluation (utils/metrics.py:39-83), at the resolution of the slot grid.  Every result is an integer, or an
 * fp32 value rounded once per step of the host chain it restates: results are the same bits on every run.
 *
 * focus_slot_segments: attn [B,T,N = He We,K] contiguous, fp32 or bf16, K innermost (the slot update's layout; rows need no
 *   alignment beyond the element's) ->
 *     seg   uint8 [B,T,N]    the arg-max slot of each cell, the LOWEST index among equal maxima (NaN scores: unspecified);
 *     stats int32 [B,T,K,5]  (count, xmin, ymin, xmax, ymax) of each slot in each frame in cell units, cell n at
 *                            y = n / We, x = n % We; a slot without a cell in the frame: (0, We, He, -1, -1).
 *   attn is read once.  A frame split over several workgroups is combined by integer add / min / max atomics into stats
 *   that a first launch set to the empty value.  Status, in this order: FOCUS_ERR_NULL; FOCUS_ERR_SHAPE (B or T < 0, K < 1,
 *   K > 32, He < 1, We < 1, He We K >= 2^31); FOCUS_ERR_DTYPE; FOCUS_ERR_ALIGN (attn not element-aligned, stats not 4-byte
 *   aligned); FOCUS_OK without a launch for B T == 0.
 *
 * focus_slot_boxes: stats -> boxes fp32 [B,T,O,4] in the orvit_bboxes encoding (cx, cy, w, h in [0,1]; all-zero row = no
 *   object) and slot_ids int32 [B,O], one launch.  Per clip: area[k] = sum_t count[b,t,k]; with drop_largest the slot of
 *   the largest area (ties: lowest index; the background) is removed; of the others with area > 0 the O largest are kept
 *   (ties: lowest index) and written in ASCENDING SLOT INDEX, so object o is one slot in every frame; objects beyond the
 *   kept ones are zero rows with slot_ids = -1.  With sx = W / We, sy = H / He (both must divide), the box of a kept slot
 *   in a frame is the pixel box (xmin sx, ymin sy, xmax sx + sx - 1, ymax sy + sy - 1) in fp32 -- masks_to_boxes
 *   (utils/box_ops.py:72-96) of the nearest-upsampled mask -- put through datasets/utils.boxes_to_orvit_format: IEEE
 *   division by W or H, clip to [0,1], cx = (x0+x1)/2, cy = (y0+y1)/2, w = x1-x0, h = y1-y0, a zero row when w <= 0.05 or
 *   h <= 0.05.  A slot without a cell in a frame gives a zero row there (masks_to_boxes itself returns (1e8, 1e8, 0, 0)).
 *   Status: FOCUS_ERR_NULL; FOCUS_ERR_SHAPE (B, T or O < 0, K < 1, K > 32, He, We, H or W < 1, H % He or W % We != 0,
 *   T He We >= 2^31, H or W > 2^24); FOCUS_ERR_ALIGN (4 bytes); FOCUS_OK without a launch for B == 0 or O == 0.
 *
 * focus_seg_contingency: seg uint8 [B,T,He We] and truth [B,T,S,1,H,W] (uint8 / bool, or fp32 when truth_is_f32; non-zero =
 *   member, masks may overlap) -> table int32 [B, S - first_segment, K],
 *     table[b,s,k] = #{(t,y,x): truth[b,t,s+first_segment,y,x] != 0 and seg[b,t,(y/sy) We + x/sx] == k}.
 *   The table is zeroed on the stream first: the call leaves exactly these counts.  Truth is read once, 16 bytes per lane
 *   when W allows it; counts are summed per wave in LDS, then one integer atomic per non-zero bin per workgroup.  A seg
 *   value >= K counts nowhere.  Status: FOCUS_ERR_NULL; FOCUS_ERR_SHAPE (B or T < 0, S, H, W, He, We or K < 1, K > 32,
 *   first_segment < 0, S - first_segment < 1, H % He or W % We != 0, T H W >= 2^31, B (S - first_segment) >= 2^26);
 *   FOCUS_ERR_ALIGN (table or fp32 truth not 4-byte aligned); FOCUS_OK without a launch for B == 0.
 * ----------------------------------------------------------------------------------------------*/
int focus_slot_segments(const void* attn, int dtype, int B, int T, int He, int We, int K, uint8_t* seg, int32_t* stats,
                        void* stream);
int focus_slot_boxes(const int32_t* stats, int B, int T, int K, int He, int We, int H, int W, int O, int drop_largest,
                     float* boxes, int32_t* slot_ids, void* stream);
int focus_seg_contingency(const uint8_t* seg, const void* truth, int truth_is_f32, int B, int T, int S, int H, int W, int He,
                          int We, int K, int first_segment, int32_t* table, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Step and test statistics on the device (step_stats.hip): what the loops of tools/train_net.py:123-269, :311-470 and
 * tools/test_net.py:85-128 do with the predictions, without a host round trip.  Counts are integers (integer atomics:
 * the same in any arrival order); the double sums are touched by exactly one thread per launch; no float atomics.
 *
 * focus_topk_stats: adds one batch into an accumulator that stays on the device.  No argument varies from step to step
 *   (the step counter lives in the accumulator), so the launch can sit inside a captured step.
 *     heads in {0, 1, 2}; per head h: logits [B, V_h], row stride ld_h in elements, dtype_h FOCUS_F32 or FOCUS_BF16, and
 *     labels: int64 [B] (dense_labels == 0) or dense fp32 [B, V_h] with row stride ldl_h (dense_labels != 0, the mixup
 *     targets).  nk values k0 < k1 < ... (nk <= 4; the others are not looked at).  loss0..2: device fp32 scalars, any may
 *     be NULL.  acc_i: int64 [16] = steps, samples, nan (0 / 1), nan_step, correct[3][4] (row h, column = index into ks;
 *     row 2 = every head); acc_f: float64 [8] = loss_sum[3], loss_weighted[3], 2 unused.  Both start as zeros.
 *   Order: entry (x, i) beats (y, j) if exactly one of x, y is NaN and it is x; otherwise if x > y, or x == y and i < j
 *     (NaN greatest as in torch.topk, ties to the lowest index as in focus_greedy_next).  A row is correct at k when
 *     fewer than k entries of its row beat the label's entry; a label outside [0, V) is never correct.
 *   Dense labels (train_net.py:123-149): first = the greatest entry of the label row by that order, second = the greatest
 *     of the rest (several NaNs in a label row: the lowest index first).  The row is scored as if pred[first] = pred[first] +
 *     pred[second], the sum formed in fp32 and rounded once to the logits' dtype, and pred[second] = 0; the label is first.
 *     The logits are not written.
 *   correct[0], correct[1] count per head; correct[2] counts rows correct in every head at that k (with one head it equals
 *     correct[0]).  steps += 1, samples += B; for each non-NULL loss_i: loss_sum[i] += (double)loss_i, loss_weighted[i] +=
 *     (double)loss_i * B, by one thread, so the sums are the bits of the same double sums formed on the host in step order.
 *     If loss0 is NaN (inf passes) and nan == 0: nan = 1, nan_step = the value steps had before this launch.
 *     heads == 0 updates only these scalars.
 *   Status, before any launch (a refused call writes nothing): FOCUS_ERR_NULL (acc_i or acc_f); FOCUS_ERR_SHAPE (heads
 *     outside 0..2); FOCUS_ERR_NULL (logits or labels of a head in use); with heads > 0 FOCUS_ERR_SHAPE (nk outside 1..4, a
 *     k < 1 or not above the one before, the largest k above some V_h, V_h < 1, V_h < 2 with dense labels, ld_h < V_h, ldl_h <
 *     V_h with dense labels) and FOCUS_ERR_DTYPE (logits neither fp32 nor bf16); FOCUS_OK without a launch for B <= 0.
 *
 * focus_view_accumulate: the multi-view ensembling of meters.py:300-332 / :1181-1201 for one head.  preds [n, C] fp32 or
 *   bf16 with row stride ld, clip_ids and labels int64 [n] on the device; row i belongs to video clip_ids[i] / num_clips.
 *   video_preds fp32 [num_videos, C], video_labels and clip_count int64 [num_videos], flag int32 [1] (sticky: bits are only
 *   ever set).  Rows of the batch that share a video are folded in ascending row order by one owner (the first such row),
 *   starting from the table's row: FOCUS_VIEW_SUM gives the bits of the reference's per-clip fp32 loop whatever the batch
 *   split, FOCUS_VIEW_MAX is torch.max (a NaN stays).  Walking its rows in the same order the owner sets bit 0 of flag when
 *   a clip's label differs from a non-zero label stored for the video (the label is written either way) and adds the rows
 *   to clip_count.  A clip id outside [0, num_videos * num_clips) is skipped and sets bit 1.
 *   Status, before any launch: FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE (num_clips < 1, num_videos < 0, C < 1,
 *     C > 65535 * 256, ld < C, an unknown mode); FOCUS_ERR_DTYPE; FOCUS_OK without a launch for n <= 0.
 * ----------------------------------------------------------------------------------------------*/
enum focus_view_mode { FOCUS_VIEW_SUM = 0, FOCUS_VIEW_MAX = 1 };
int focus_topk_stats(int heads, int B, const void* logits0, int dtype0, int V0, int64_t ld0, const void* labels0, int64_t ldl0,
                     const void* logits1, int dtype1, int V1, int64_t ld1, const void* labels1, int64_t ldl1, int dense_labels,
                     int nk, int k0, int k1, int k2, int k3, const float* loss0, const float* loss1, const float* loss2,
                     int64_t* acc_i, double* acc_f, void* stream);
int focus_view_accumulate(const void* preds, int dtype, int n, int C, int64_t ld, const int64_t* clip_ids, const int64_t* labels,
                          int num_clips, int num_videos, int mode, float* video_preds, int64_t* video_labels,
                          int64_t* clip_count, int32_t* flag, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Random erasing (random_erase.hip; datasets/random_erasing.py of the reference, the last step of Ssv2._aug_frame): rectangles
 * of a batch of normalised clips are overwritten IN PLACE, in one launch.  x is the tensor focus_clip_sample wrote and is
 * addressed the same way: element (b, c, t, y, x) lives at  b*sb + c*sc + t*st + y*W + x  (strides in elements, rows and
 * planes of H x W dense), so one entry point serves [B,C,T,H,W] and [B,T,C,H,W], fp32 and bf16.
 *
 * `items`: DEVICE array of n_items descriptors owned by the caller.  An item erases the rectangle [top, top+h) x
 * [left, left+w) of every channel of the frames [t0, t1) of clip `clip`.  The items of one clip are CONTIGUOUS in the table
 * and stand in the order the reference writes them: where rectangles of one clip overlap, every pixel gets the value of the
 * LAST item of its clip that covers it -- the thread that owns a pixel of item i looks at the up to max_per_clip - 1 items
 * behind i, and leaves the pixel alone when one of them has the same clip and covers it too.  So the result does not depend on
 * scheduling; max_per_clip is the largest number of items any clip has in the table (1: nothing is scanned).  `ord` is the
 * item's ordinal within its clip; it feeds the generator and nothing else.
 *
 * What is written, by mode:
 *   FOCUS_ERASE_CONST  +0.0
 *   FOCUS_ERASE_RAND   one N(0,1) value per (item, frame, channel):  zc(ord, clip, t, c, 0xffffffff)
 *   FOCUS_ERASE_PIXEL  one N(0,1) value per (item, frame, channel, y, x):  with p = (y << 16) | (x >> 1),
 *                      zc(ord, clip, t, c, p) in an even column x and zs(ord, clip, t, c, p) in an odd one
 * with the build-owned counter-based generator (mix32 = lowbias32, as in gumbel.hip; all integer arithmetic mod 2^32):
 *     k  = mix32(mix32(mix32(seed[0] ^ clip) + ord * 0x9E3779B9) ^ t) + c * 0x9E3779B9
 *     ha = mix32(mix32(k) ^ p),   hb = mix32(ha ^ seed[1])
 *     u1 = ((ha >> 9) + 0.5) / 2^23  in (0, 1),   u2 = (hb >> 8) / 2^24  in [0, 1)          (both exact in fp32)
 *     r  = sqrtf(-2 logf(u1)),   zc = r * cospif(2 u2),   zs = r * sinpif(2 u2)              (Box-Muller, fp32: the two
 *                                                                   values of one draw are independent N(0,1) values)
 * t, c, y, x are LOGICAL coordinates of the tensor, so both layouts, both dtypes and any launch geometry give the same
 * number; bf16 is one round-to-nearest-even of the fp32 value.  |z| <= sqrt(2 ln 2^24) = 5.77.  `seed`: two 32-bit words on
 * the DEVICE (not read for FOCUS_ERASE_CONST, where it may be NULL).  The reference draws the fill from torch's CPU generator:
 * the distribution here is the reference's, the draws are not (as for the decoder's dropout, focus_dropout_add).
 *
 * The kernel only writes: it reads the table and the seed, and neither reads nor writes a byte of x outside the rectangles.
 * Rows start at an arbitrary `left`: the 16-byte-aligned body of a row is written with 16-byte stores, its ends element by
 * element.  No workspace, no atomics: the same arguments give the same bits.
 *
 * The table lives on the device, so this entry point cannot judge it.  The kernel clamps every rectangle to [0,H) x [0,W)
 * and every frame range to [0,T), and skips an item that is empty afterwards or whose clip is outside [0,B), so a bad
 * descriptor cannot write outside the tensor (focus_amd.ops.random_erase_ raises ValueError for every such item instead).
 *
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (x or items is NULL; seed is
 * NULL in a mode that draws); FOCUS_OK without a launch for n_items <= 0; FOCUS_ERR_SHAPE (an unknown mode; B, T, C, H or W
 * < 1; H or W > 32768; T, C or n_items > 65535; max_per_clip outside [1, FOCUS_ERASE_MAX_PER_CLIP]; sb < 1, sc < H*W or
 * st < H*W); FOCUS_ERR_DTYPE (neither FOCUS_F32 nor FOCUS_BF16); FOCUS_ERR_ALIGN (x not aligned to its element size).
 * ----------------------------------------------------------------------------------------------*/
#define FOCUS_ERASE_MAX_PER_CLIP 64
enum focus_erase_mode { FOCUS_ERASE_CONST = 0, FOCUS_ERASE_RAND = 1, FOCUS_ERASE_PIXEL = 2 };
typedef struct focus_erase_item {
    int32_t clip, t0, t1, top, left, h, w, ord;
} focus_erase_item;
int focus_random_erase(void* x, int dtype, int B, int T, int C, int H, int W, int64_t sb, int64_t sc, int64_t st,
                       const focus_erase_item* items, int n_items, int max_per_clip, int mode, const void* seed,
                       void* stream);

/* -------------------------------------------------------------------------------------------------
 * STEVE epoch visualisation (slot_vis.hip; slowfast/utils/slot_misc.py:16-35 of the reference): the video that
 * visualize() hands to add_video -- per frame torch.cat((video, recon_dvae, recon_tf, attns)) put through torchvision's
 * make_grid(tiles, nrow = K + 3, padding = 2, pad_value = 0.8) -- written whole in ONE launch.
 *
 * out [T,3,Hg,Wg] dense, Hg = rows (H + 2) + 2, Wg = (K + 3) (W + 2) + 2.  The canvas is 0.8f; tile (r, j) of frame t lies
 * at rows r (H + 2) + 2 ... + H and columns j (W + 2) + 2 ... + W, for r < rows and j < K + 3:
 *     j = 0: video[r,t]    j = 1: recon[r,t]    j = 2: gen[r,t]    j = 3 + k: the overlay of slot k.
 * video [B,T,3,H,W], recon [B,T,3,H,W], gen [Bg,T,3,H,W]: dense, each FOCUS_F32 or FOCUS_BF16 by its own dtype argument
 * (bf16 widens exactly, which is what torch.cat's type promotion does).  `slots` is the slot source, by slot_form:
 *   FOCUS_SLOT_FORM_VIS  attns_vis [B,T,K,3,H,W] fp32, as STEVE.forward / encode return it; the tiles are copied.  He and We
 *                        are not looked at.
 *   FOCUS_SLOT_FORM_RAW  attn [B,T,He We,K] fp32 or bf16, as the slot update leaves it (K innermost), He | H and We | W.
 *                        With sy = H / He, sx = W / We, v = video[r,t,c,y,x] and a = attn[r,t,(y / sy) We + x / sx,k], the
 *                        pixel is  fadd(fmul(v, a), fsub(1, a))  in fp32, each of the three rounded on its own -- the
 *                        bits of steve.py:314-319 (nearest upsampling by repeat_interleave, then mul, rsub, add) without
 *                        any [B,T,K,...] tensor.  No FMA: a single rounding changes about one result in ten.
 * out_type FOCUS_VIS_OUT_F32 writes those fp32 values: bit-equal to the reference's composition.  FOCUS_VIS_OUT_U8 writes
 * what torch.utils.tensorboard (summary.py:video) makes of them on the host, (x * 255).clip(0, 255).astype(uint8) with the
 * product rounded to fp32: the conversion TRUNCATES, a NaN becomes 0, the canvas comes out as 204.
 *
 * The launch is driven from the output: every element of out is written exactly once (vector stores in the aligned body of
 * a canvas row, element stores at its two ends -- Wg is rarely a multiple of 4), nothing outside out is written, nothing
 * is read but the tiles.  No workspace, no atomics: the same arguments give the same bits.
 *
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (video, recon, gen, slots
 * or out is NULL); FOCUS_ERR_SHAPE (an unknown slot_form; C != 3; K outside 1..32; B, Bg, H or W < 1; T < 0; rows < 0 or
 * rows > min(B, Bg); in the raw form He or We < 1, H % He != 0 or W % We != 0; T 3 Hg Wg >= 2^31); FOCUS_ERR_DTYPE (a source
 * neither FOCUS_F32 nor FOCUS_BF16; attns_vis not FOCUS_F32; an unknown out_type); FOCUS_ERR_ALIGN (a source, or an fp32
 * out, not aligned to its element size); FOCUS_OK without a launch for rows == 0 or T == 0.
 * ----------------------------------------------------------------------------------------------*/
enum focus_slot_form { FOCUS_SLOT_FORM_VIS = 0, FOCUS_SLOT_FORM_RAW = 1 };
enum focus_vis_out { FOCUS_VIS_OUT_F32 = 0, FOCUS_VIS_OUT_U8 = 1 };
int focus_slot_vis_grid(const void* video, int dtype_video, const void* recon, int dtype_recon, const void* gen,
                        int dtype_gen, const void* slots, int dtype_slots, int slot_form, int B, int Bg, int T, int C, int H,
                        int W, int K, int He, int We, int rows, void* out, int out_type, void* stream);

/* -------------------------------------------------------------------------------------------------
 * The multi-label route (multilabel.hip; DATA.MULTI_LABEL of the reference: slowfast/models/losses.py:91-92,
 * slowfast/utils/meters.py:275-334, :390-394 and :1275-1299).  No float atomics and no data-dependent order in any of the
 * three: the same arguments give the same bits.
 *
 * focus_bce_rows: nn.BCEWithLogitsLoss (FOCUS_BCE_LOGITS) and nn.BCELoss (FOCUS_BCE_PROBS), value and gradient in one launch.
 *   x [R,C] fp32 with row stride ldx, targets y [R,C] fp32 with row stride ldy (any value in [0,1], not only 0 / 1).
 *   loss_rows [R] fp32: the sum of the row's elements -- thread t of the row's 256-thread workgroup adds elements t, t + 256, ...
 *   in ascending order, the 256 partial sums are folded by halving.  dx [R,C] fp32 with row stride lddx: grad_scale times the
 *   derivative of that sum; the caller passes 1 / (R C) for the mean and 1 for the sum.  Per element, every operation in fp32:
 *     logits  e = max(x, 0) - x y + log1pf(expf(-|x|))                      de/dx = sigmoid(x) - y, sigmoid from the same expf
 *     probs   e = -(y max(logf(x), -100) + (1 - y) max(log1pf(-x), -100))   de/dx = (x - y) / max((1 - x) x, 1e-12f)
 *   The second line is ATen's clamp rule.  expf, logf and log1pf are the accurate library functions.  Probabilities outside
 *   [0,1] (ATen raises) give NaN.  Elements of x, y and dx past C in a row are neither read nor written.
 *   Status, in this order, before any launch: FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE (R < 0, C < 1, a row stride below C,
 *     an unknown mode); FOCUS_OK without a launch for R == 0.
 *
 * focus_view_accumulate_dense: focus_view_accumulate for TestMeter(multi_label=True).  The same ownership rule (the rows of
 *   a batch that share a video are folded in ascending row order by the first of them, starting from the table's row), the
 *   same modes, clip_count and sticky flag (bit 1: a clip id outside [0, num_videos num_clips)).  What differs: labels is
 *   dense fp32 [n,C] with row stride ldl and video_labels fp32 [num_videos,C]; walking its rows the owner sets bit 0 of
 *   flag when the row stored for the video has an element > 0 (for labels >= 0: a sum > 0, the reference's test) and is not
 *   element-wise equal to the clip's row; the clip's row is stored either way.  The table's first value is the caller's
 *   business: the reference fills -1e10, and with FOCUS_VIEW_SUM fp32 then swallows every score added to it.
 *   Status, before any launch: FOCUS_ERR_NULL (any pointer); FOCUS_ERR_SHAPE (num_clips < 1, num_videos < 0, C < 1, ld < C,
 *     ldl < C, an unknown mode, C > 65535 * 256); FOCUS_ERR_DTYPE (preds neither fp32 nor bf16); FOCUS_OK without a launch
 *     for n <= 0.
 *
 * focus_average_precision: get_map for a table on the device.  scores [N,C] fp32 with row stride lds, labels [N,C] fp32
 *   with row stride ldl, 0 or 1.  For class c with positives P = {i : y_i == 1}, scikit-learn's step-wise average precision
 *   (tied scores form one threshold) is
 *       AP_c = (1 / |P|) sum_{i in P} TP_i / CNT_i,    CNT_i = #{j : s_j >= s_i},  TP_i = #{j : s_j >= s_i, y_j == 1}:
 *   the threshold s_i contributes (its positives / |P|) x (its precision TP / CNT), once per positive at it.  The counts are
 *   integers and exact; nothing is sorted.  Order of the double sum: rows in tiles of 256; per tile the 256 quotients (0 for
 *   a row that is no positive) are folded by halving (slot s += slot s + h, h = 128, ..., 1), the tiles' sums are added in
 *   ascending order, the total is divided by |P|.
 *   npos [C] int64: the number of non-zero labels of the class (its positives, for 0 / 1 labels).  A class with npos == 0 is
 *   left out, as get_map drops all-zero label columns, and gets ap 0.  ap [C] float64.  summary float64 [2]: the mean of
 *   ap over the kept classes, added in ascending class order by one thread (0 when none is kept), and their number.
 *   flag int32 [1], OVERWRITTEN: bit 0 a label of a kept class is neither 0 nor 1; bit 1 a score of a kept class is not
 *   finite; bit 2 no class kept.  scikit-learn raises for bits 1 and 2, and get_map then returns 0.
 *   workspace: focus_average_precision_workspace_bytes(N, C) bytes, 8-byte aligned; two launches on the caller's stream.
 *   Status, in this order, before any launch: FOCUS_ERR_NULL (scores, labels, npos, ap, summary, flag); FOCUS_ERR_SHAPE
 *     (N < 0, C < 1, C > 65535, a row stride below C, ceil(N / 256) C >= 2^23); FOCUS_OK without a launch, NOTHING written,
 *     for N == 0; FOCUS_ERR_NULL (workspace); FOCUS_ERR_ALIGN; FOCUS_ERR_WORKSPACE.
 * ----------------------------------------------------------------------------------------------*/
enum focus_bce_mode { FOCUS_BCE_LOGITS = 0, FOCUS_BCE_PROBS = 1 };
int focus_bce_rows(const float* x, int64_t ldx, const float* y, int64_t ldy, int R, int C, int mode, float grad_scale,
                   float* loss_rows, float* dx, int64_t lddx, void* stream);
int focus_view_accumulate_dense(const void* preds, int dtype, int n, int C, int64_t ld, const int64_t* clip_ids,
                                const float* labels, int64_t ldl, int num_clips, int num_videos, int mode, float* video_preds,
                                float* video_labels, int64_t* clip_count, int32_t* flag, void* stream);
size_t focus_average_precision_workspace_bytes(int N, int C);
int focus_average_precision(const float* scores, int64_t lds, const float* labels, int64_t ldl, int N, int C, int64_t* npos,
                            double* ap, double* summary, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * The AVA evaluation (ava_eval.hip; PascalBoxes mAP@0.5IOU of the reference: slowfast/utils/ava_eval_helper.py:174-287,
 * ava_evaluation/per_image_evaluation.py:261-352, object_detection_evaluation.py:640-830, metrics.py:21-125).  No float
 * atomics (the counters are integers) and no data-dependent order: the same arguments give the same bits.
 *
 * focus_ava_match: the greedy match per (image, class).
 *   boxes [K,4] fp32 (x1, y1, x2, y2), the detection rows in arrival order.  A row with not (y1 < y2 and x1 < x2) is
 *   invalid and is not judged.
 *   Groups: the rows of one image.  grp_off int64 [n_groups + 1] are offsets into det_rows int64 [K], which lists the rows
 *   of group 0, then of group 1, ..., each group in ascending row (= arrival) order; rows of excluded images are listed
 *   nowhere, so fewer than K entries may be in use.  grp_image int64 [n_groups]: the ground-truth image of the group,
 *   or a negative value when the image has no ground truth (all its rows are false positives).
 *   Ground truth: gt_off int64 [n_images + 1] offsets into gt_class int32 [.] (1-based class ids) and gt_boxes float64 [.,4]
 *   (x1, y1, x2, y2), the rows of an image in file order.
 *   whitelist uint8 [C]: class c (0-based; class id c + 1) is evaluated when its byte is non-zero.
 *   Per (group, whitelisted class) the valid rows are walked in order.  In float64, boxes widened,
 *       area = (y2 - y1) (x2 - x1)    ih = max(min(y2, y2') - max(y1, y1'), 0)    iw likewise    inter = ih iw
 *       iou = inter / (area + area' - inter)
 *   against the ground-truth rows of that class in the image; the FIRST maximum is the candidate; the row is a true positive
 *   when iou >= 0.5 and the candidate has not been taken, and takes it; otherwise it is a false positive.
 *   out uint8 [K,C] with row stride ldo: 1 false positive, 2 true positive, written for judged (row, class) pairs only;
 *   every other byte is left as the caller set it (0: not evaluated).  counts int64 [2,C]: the judged rows and the true
 *   positives per class are ADDED.  flag int32 [1], sticky (OR-ed): bit 0 an (image, class) has more than 64 ground-truth
 *   rows, none of its rows is judged; bit 1 an index of the group tables is out of range, the entry is skipped.
 *   One launch.  Status, in this order: FOCUS_ERR_NULL (out, counts, flag, whitelist; with K > 0 boxes or a group table;
 *     with n_images > 0 a ground-truth table); FOCUS_ERR_SHAPE (K < 0, C < 1, C > 65535 * 256, n_groups < 0 or >= 2^31,
 *     n_images < 0, ldo < C); FOCUS_OK without a launch for K == 0 or n_groups == 0.  The scores are not an argument: the
 *     match does not look at them.
 *
 * focus_voc_ap: the VOC average precision per class.  scores [N,C] fp32 or bf16 with row stride lds, bytes uint8 [N,C] with
 *   row stride ldb as focus_ava_match writes them (0 not evaluated, 2 true positive, anything else false positive), n_gt
 *   int64 [C] the ground-truth rows per class, total_gt >= sum of n_gt (a host value: it sizes the workspace).
 *   The evaluated rows of class c are ordered by descending score, equal scores by DESCENDING row index.  With pos_j the
 *   0-based rank of the j-th true positive in that order (j = 1..m), n = n_gt[c]:
 *       p_j = j / (pos_j + 1)    env_j = max_{j' >= j} p_j'    AP_c = sum_j (j / n - (j - 1) / n) env_j        (float64)
 *   The ranks are counted, nothing is sorted.  Order of the sum: with L = ceil(m / 256), part k (k = 0..255) adds the terms
 *   of j = min(k L + L, m) down to k L + 1, in descending j, starting from 0; the 256 parts are folded by halving (part s +=
 *   part s + h for h = 128, ..., 1).
 *   ap [C] float64: NaN for n == 0, 0 without an evaluated row.  summary float64 [2]: the mean of ap over the classes with
 *   n > 0 (NaN when there is none), added in ascending class order by one thread, and their number.
 *   flag int32 [1], OVERWRITTEN: bit 0 a score of an evaluated row is not finite; bit 1 more true positives than n in a
 *   class with n > 0 (the reference's ValueError), its ap is NaN and it is left out of the mean; bit 2 the n_gt add up to more than
 *   total_gt, the classes without room likewise.
 *   workspace: focus_voc_ap_workspace_bytes(N, C, total_gt) bytes, 8-byte aligned (it also holds a class-major copy of the
 *   evaluated scores: 5 bytes per (row, class)); five launches on the caller's stream.
 *   Status, in this order: FOCUS_ERR_NULL (n_gt, ap, summary, flag, workspace; scores or bytes with N > 0); FOCUS_ERR_SHAPE
 *     (N < 0, N > 2^31 - 257, ceil(N / 256) C >= 2^31, C < 1, C > 65535, total_gt < 0, a row stride below C); FOCUS_ERR_DTYPE; FOCUS_ERR_ALIGN;
 *     FOCUS_ERR_WORKSPACE.
 *     N == 0 is scored like any table: every class with ground truth gets 0.
 * ----------------------------------------------------------------------------------------------*/
int focus_ava_match(const float* boxes, int64_t K, int C, const int64_t* grp_off, const int64_t* det_rows,
                    const int64_t* grp_image, int64_t n_groups, const int64_t* gt_off, const int32_t* gt_class,
                    const double* gt_boxes, int64_t n_images, const uint8_t* whitelist, uint8_t* out, int64_t ldo,
                    int64_t* counts, int32_t* flag, void* stream);
size_t focus_voc_ap_workspace_bytes(int64_t N, int C, int64_t total_gt);
int focus_voc_ap(const void* scores, int dtype, int64_t lds, const uint8_t* bytes, int64_t ldb, int64_t N, int C,
                 const int64_t* n_gt, int64_t total_gt, double* ap, double* summary, int32_t* flag, void* workspace,
                 size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Pooling attention in token layout (token_pool.hip; attention.py:16-50, the attention_pool of MViT: a depth-wise Conv3d,
 * MaxPool3d or AvgPool3d over the (T, H, W) grid of the tokens, then a LayerNorm per head).
 *
 * x is [B, cls + T*H*W, C] rows (sample stride x_batch_stride, row stride x_row_stride, in elements: a strided view is read in
 * place); the columns are C / head_dim heads of head_dim.  The row of grid cell (t, h, w) is cls + (t*H + h)*W + w; with
 * cls == 1 row 0 passes to output row 0 unpooled.  Output extents o = (i + 2p - k) / s + 1 (floor), output rows
 * cls + ot*oh*ow per sample; every output is dense.  k, s, p are in (t, h, w) order; tap = (kt*kh_ + kh)*kw_ + kw.
 *   FOCUS_POOL_CONV  y[c] = sum over the in-bounds taps of w[c % head_dim][tap] * x[c], fp32 in tap order; w is fp32
 *                    [head_dim, kt*kh*kw] (a dense Conv3d.weight [head_dim, 1, kt, kh, kw] as it stands); no bias.
 *   FOCUS_POOL_AVG   the sum over the in-bounds taps divided by kt*kh*kw (count_include_pad: padded taps count).
 *   FOCUS_POOL_MAX   the maximum over the in-bounds taps, a NaN counting as a maximum; idx [B, rows_out, C] int8 holds the
 *                    tap of the FIRST maximum in (t, h, w) order (ATen's rule); the cls row holds -1.
 * gamma, beta (both or neither; fp32 [head_dim]): every output row, the cls row included, is normalised per head_dim-wide
 *   column group from the un-rounded fp32 pooled values (biased variance, eps inside the root) -> y; the forward then also
 *   writes the pre-norm rows to `pooled` in `dtype` and mean, rstd fp32 [B*rows_out*heads]: the arguments of
 *   focus_layernorm_bwd with `pooled` viewed as [B*rows_out*heads, head_dim].  pooled, mean, rstd: all three or none (none: a forward
 *   that keeps nothing for a backward).  Without gamma and beta y holds the pooled rows and the three are not written.
 * focus_token_pool_bwd, from dpooled [B, rows_out, C] (after focus_layernorm_bwd where the forward normalised):
 *   dx [B, rows_in, C] dense (may be NULL: not formed), a gather: every element is written once, the sum over the output
 *     positions whose window covers the cell of w[c % head_dim][tap] * dpooled (max: dpooled where idx equals the tap; avg:
 *     the sum / (kt*kh*kw)); the cls row receives dpooled row 0.
 *   dw [head_dim, kt*kh*kw] fp32, OVERWRITTEN (conv only; may be NULL): the sum over samples, heads and output positions of
 *     dpooled * x[tap].  Two stages in a fixed order: block partials in `workspace` (focus_token_pool_workspace_bytes), then
 *     one reduction.  No atomics anywhere: the same inputs give the same bits.
 * Host-only helpers: focus_token_pool_blocks(d, stage) is the number of workgroups of stage 0 (forward), 1 (forward with the
 *   LayerNorm), 2 (dx) or the number of row blocks of the dw partials (3); 0 for a descriptor the kernels refuse.
 *   focus_token_pool_workspace_bytes is 0 for such a descriptor and outside conv mode.
 *
 * Limits: head_dim % 8 == 0, head_dim >= 8, C % head_dim == 0, C <= 4096; head_dim <= 128 in conv mode or with the
 *   LayerNorm; k in 1..7, s in 1..8, 0 <= p < k; kt*kh*kw <= 127 in max mode (the tap is an int8); every extent >= 1 and every
 *   output extent >= 1; B*rows*C < 2^31 for the input and the output; x_row_stride >= C.
 * Status, judged in this order before any launch (a refused call writes nothing): FOCUS_ERR_NULL (d); FOCUS_ERR_SHAPE (the
 *   limits above; B < 0; cls outside {0, 1}; an unknown mode; a negative batch stride; backward: dw outside conv mode);
 *   FOCUS_ERR_DTYPE (neither fp32 nor bf16); FOCUS_OK without a launch for B == 0; FOCUS_ERR_NULL (forward: x, y; w in conv
 *   mode; idx in max mode; gamma without beta or the reverse; some but not all of pooled, mean, rstd.  backward: dpooled; both
 *   dx and dw; with dx, w in conv mode and idx in max mode; with dw, x and workspace); FOCUS_ERR_ALIGN (a pointer not 16-byte
 *   aligned, or a stride of x that is not a multiple of 16 bytes); FOCUS_ERR_WORKSPACE (backward with dw: workspace_bytes
 *   below focus_token_pool_workspace_bytes).
 * ----------------------------------------------------------------------------------------------*/
enum focus_pool_mode { FOCUS_POOL_CONV = 0, FOCUS_POOL_MAX = 1, FOCUS_POOL_AVG = 2 };
typedef struct focus_token_pool_desc {
    int32_t B, T, H, W, C, head_dim, cls;
    int32_t k[3], s[3], p[3];
    int32_t mode, dtype;
    int64_t x_batch_stride, x_row_stride;
} focus_token_pool_desc;
int focus_token_pool_blocks(const focus_token_pool_desc* d, int stage);
size_t focus_token_pool_workspace_bytes(const focus_token_pool_desc* d);
int focus_token_pool_fwd(const focus_token_pool_desc* d, const void* x, const float* w, const float* gamma,
                         const float* beta, float eps, void* y, void* pooled, float* mean, float* rstd, void* idx,
                         void* stream);
int focus_token_pool_bwd(const focus_token_pool_desc* d, const void* dpooled, const void* x, const float* w,
                         const void* idx, void* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FOCUS_AMD_H */
