// slot_vis.hip -- the end-of-epoch STEVE visualisation (slowfast/utils/slot_misc.py:16-35 of the reference: per frame one
// torch.cat and one torchvision make_grid, i.e. a canvas fill and N (K + 3) narrow().copy_() calls) as ONE launch that writes
// the whole [T,3,Hg,Wg] video, in fp32 with the reference's bits or in the uint8 TensorBoard makes of it on the host.
//
// The launch is driven from the OUTPUT.  A workgroup owns canvas rows (t, c, y) -- so the frame, the channel, the tile row
// and whether the row is padding are workgroup-uniform and cost scalar arithmetic -- and a thread owns one 4-element chunk of
// that row whose address is aligned to the chunk (16 bytes fp32, 4 bytes uint8).  Wg is rarely a multiple of 4, so where a
// row starts relative to such an address differs from row to row: the chunks a row's two ends cut are stored element by
// element, every other one with a single vector store.  Every canvas element is written by exactly one thread, nothing
// outside the canvas is touched, nothing of the canvas is read, and there are no atomics: the same arguments give the same bits.
//
// A thread walks its 4 columns keeping (tile column, offset inside the tile, slot-grid cell) incrementally: one division pair
// per chunk, not per element.  The sources are gathered element-wise (a tile starts at column j (W + 2) + 2 of the canvas, which
// no alignment of the source rows survives); neighbouring lanes read neighbouring addresses, and in the raw form the attention
// of a cell is re-read from cache by the sx pixels and the three channels that share it.  In the uint8 form the bytes loaded
// are 4 to 8 times the bytes stored, which is why a chunk stays at 4 elements there: wider chunks spread the lanes' loads.
//
// Raw form: the overlay pixel v a + (1 - a) is three separately rounded fp32 operations (the ATen chain mul, rsub, add of
// steve.py:319).  __fmul_rn, __fsub_rn and __fadd_rn do NOT give that here: HIP's header defines them as the plain operators
// inside inline functions compiled with contraction allowed, and hipcc fused the product and the sum into one v_fmac_f32
// whether they were called directly or under a contract(off) pragma (seen in this file's assembly; the first version of the
// kernel differed from the reference for that reason).  overlay_px therefore writes the operators itself under
// `#pragma clang fp contract(off)`, which leaves v_mul_f32, v_sub_f32, v_add_f32.
#include "focus_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int VEC = 4;
constexpr int MAX_BLOCKS_X = 1 << 20;     // rows; the loops stride over the rest
constexpr int MAX_BLOCKS_Y = 64;

struct VisArgs {
    const void *video, *recon, *gen, *slots;
    int bf_video, bf_recon, bf_gen, bf_slots;
    int T, H, W, K, He, We, sy, sx, Hg, Wg;
    uint32_t nrows;                                       // T * 3 * Hg
};

__device__ __forceinline__ float ld_src(const void* p, int64_t i, int bf) {
    return bf ? bf16_to_f32(static_cast<const bf16_t*>(p)[i]) : static_cast<const float*>(p)[i];
}

// summary.py:video of torch.utils.tensorboard: (x * 255).clip(0, 255).astype(uint8) in fp32.  fmaxf drops a NaN: it becomes 0.
__device__ __forceinline__ uint32_t to_u8(float x) {
    return (uint32_t)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);      // one product: nothing to contract with
}

// v a + (1 - a), each operation rounded to fp32 on its own
__device__ __forceinline__ float overlay_px(float v, float a) {
#pragma clang fp contract(off)
    const float prod = v * a;
    const float rest = 1.0f - a;
    return prod + rest;
}

__device__ __forceinline__ void store_one(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_one(uint8_t* p, float v) { *p = (uint8_t)to_u8(v); }
__device__ __forceinline__ void store_vec(float* p, const float (&v)[VEC]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_vec(uint8_t* p, const float (&v)[VEC]) {
    *reinterpret_cast<uint32_t*>(p) = to_u8(v[0]) | (to_u8(v[1]) << 8) | (to_u8(v[2]) << 16) | (to_u8(v[3]) << 24);
}

template <typename O, int RAW>
__global__ __launch_bounds__(THREADS) void slot_vis_grid_kernel(VisArgs a, O* __restrict__ out) {
    const int H = a.H, W = a.W, Wg = a.Wg;
    const int nchunk = (Wg + VEC - 1) / VEC + 1;                       // aligned chunks a row of Wg elements can touch
    for (uint32_t row = blockIdx.x; row < a.nrows; row += gridDim.x) {
        const int y = (int)(row % (uint32_t)a.Hg);
        const int tc = (int)(row / (uint32_t)a.Hg), c = tc % 3, t = tc / 3;
        // y + H = qy (H + 2) + ty: canvas rows 0, 1 give qy = 0, ty >= H; tile row r = qy - 1 holds ty < H, its padding ty >= H
        const int qy = (y + H) / (H + 2), ty = (y + H) - qy * (H + 2);
        const bool row_pad = ty >= H;
        const int r = qy - 1;
        O* orow = out + (int64_t)row * Wg;
        // chunk j holds the columns [lo, lo + VEC); orow + lo is aligned to the chunk (al: how far column 0 is past such an address)
        const int al = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(O)) & (uintptr_t)(VEC - 1));
        const int64_t frame = (int64_t)r * a.T + t;                    // only used when !row_pad, where 0 <= r < rows
        const int64_t plane = ((frame * 3 + c) * H + ty) * W;          // row ty of channel c of video / recon / gen [r, t]
        int64_t slot_row = 0, slot_step = 0;
        if (RAW) {
            slot_row = (frame * a.He * a.We + (int64_t)(ty / a.sy) * a.We) * a.K;          // attn[r, t, cy We, 0]
        } else {
            slot_step = (int64_t)3 * H * W;                                                // from slot k to slot k + 1
            slot_row = frame * a.K * slot_step + ((int64_t)c * H + ty) * W;                // attns_vis[r, t, 0, c, ty, 0]
        }
        for (int j = blockIdx.y * THREADS + threadIdx.x; j < nchunk; j += gridDim.y * THREADS) {
            const int lo = j * VEC - al;
            const int xs = max(lo, 0), xe = min(lo + VEC, Wg);
            if (xs >= xe) continue;
            float v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = 0.8f;
            if (!row_pad) {
                // x + W = qx (W + 2) + tx, as for the rows; cx, rx: the cell column of tx and how far tx is into it
                int qx = (xs + W) / (W + 2), tx = (xs + W) - qx * (W + 2);
                int cx = 0, rx = 0;
                if (RAW) {
                    cx = tx / a.sx;
                    rx = tx - cx * a.sx;
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int x = lo + e;
                    if (x < xs || x >= xe) continue;
                    if (tx < W) {
                        const int col = qx - 1;                        // 0 <= col < K + 3 because x < Wg
                        if (col == 0) {
                            v[e] = ld_src(a.video, plane + tx, a.bf_video);
                        } else if (col == 1) {
                            v[e] = ld_src(a.recon, plane + tx, a.bf_recon);
                        } else if (col == 2) {
                            v[e] = ld_src(a.gen, plane + tx, a.bf_gen);
                        } else if (RAW) {
                            const float px = ld_src(a.video, plane + tx, a.bf_video);
                            const float w = ld_src(a.slots, slot_row + (int64_t)cx * a.K + (col - 3), a.bf_slots);
                            v[e] = overlay_px(px, w);
                        } else {
                            v[e] = static_cast<const float*>(a.slots)[slot_row + (col - 3) * slot_step + tx];
                        }
                    }
                    if (++tx == W + 2) {
                        tx = 0;
                        ++qx;
                        cx = rx = 0;
                    } else if (RAW && ++rx == a.sx) {
                        rx = 0;
                        ++cx;
                    }
                }
            }
            if (xs == lo && xe == lo + VEC) {
                store_vec(orow + lo, v);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (lo + e >= xs && lo + e < xe) store_one(orow + lo + e, v[e]);
            }
        }
    }
}

}  // namespace

extern "C" int focus_slot_vis_grid(const void* video, int dtype_video, const void* recon, int dtype_recon, const void* gen,
                                   int dtype_gen, const void* slots, int dtype_slots, int slot_form, int B, int Bg, int T, int C,
                                   int H, int W, int K, int He, int We, int rows, void* out, int out_type, void* stream) {
    if (!video || !recon || !gen || !slots || !out) return FOCUS_ERR_NULL;
    if (slot_form != FOCUS_SLOT_FORM_VIS && slot_form != FOCUS_SLOT_FORM_RAW) return FOCUS_ERR_SHAPE;
    if (C != 3 || K < 1 || K > 32 || B < 1 || Bg < 1 || T < 0 || H < 1 || W < 1 || rows < 0 || rows > B || rows > Bg)
        return FOCUS_ERR_SHAPE;
    const bool raw = slot_form == FOCUS_SLOT_FORM_RAW;
    if (raw && (He < 1 || We < 1 || H % He != 0 || W % We != 0)) return FOCUS_ERR_SHAPE;
    const int64_t Hg = (int64_t)rows * ((int64_t)H + 2) + 2, Wg = ((int64_t)K + 3) * ((int64_t)W + 2) + 2;
    if (Hg >= ((int64_t)1 << 31) || Wg >= ((int64_t)1 << 31) || (double)T * 3.0 * (double)Hg * (double)Wg >= 2147483648.0)
        return FOCUS_ERR_SHAPE;                                       // the product is far below 2^53 here: exact in double
    for (int dt : {dtype_video, dtype_recon, dtype_gen, dtype_slots})
        if (dt != FOCUS_F32 && dt != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (!raw && dtype_slots != FOCUS_F32) return FOCUS_ERR_DTYPE;
    if (out_type != FOCUS_VIS_OUT_F32 && out_type != FOCUS_VIS_OUT_U8) return FOCUS_ERR_DTYPE;
    if (!focus_aligned(video, focus_esize(dtype_video)) || !focus_aligned(recon, focus_esize(dtype_recon)) ||
        !focus_aligned(gen, focus_esize(dtype_gen)) || !focus_aligned(slots, focus_esize(dtype_slots)) ||
        (out_type == FOCUS_VIS_OUT_F32 && !focus_aligned(out, 4)))
        return FOCUS_ERR_ALIGN;
    if (rows == 0 || T == 0) return FOCUS_OK;
    VisArgs a;
    a.video = video; a.recon = recon; a.gen = gen; a.slots = slots;
    a.bf_video = dtype_video == FOCUS_BF16; a.bf_recon = dtype_recon == FOCUS_BF16; a.bf_gen = dtype_gen == FOCUS_BF16;
    a.bf_slots = dtype_slots == FOCUS_BF16;
    a.T = T; a.H = H; a.W = W; a.K = K;
    a.He = raw ? He : 1; a.We = raw ? We : 1; a.sy = raw ? H / He : 1; a.sx = raw ? W / We : 1;
    a.Hg = (int)Hg; a.Wg = (int)Wg;
    a.nrows = (uint32_t)((int64_t)T * 3 * Hg);
    const int64_t by = cdiv64((Wg + VEC - 1) / VEC + 1, THREADS);
    const dim3 grid((unsigned)(a.nrows > (uint32_t)MAX_BLOCKS_X ? MAX_BLOCKS_X : a.nrows),
                    (unsigned)(by > MAX_BLOCKS_Y ? MAX_BLOCKS_Y : by));
    hipStream_t s = (hipStream_t)stream;
    if (out_type == FOCUS_VIS_OUT_U8) {
        if (raw) slot_vis_grid_kernel<uint8_t, 1><<<grid, THREADS, 0, s>>>(a, (uint8_t*)out);
        else slot_vis_grid_kernel<uint8_t, 0><<<grid, THREADS, 0, s>>>(a, (uint8_t*)out);
    } else {
        if (raw) slot_vis_grid_kernel<float, 1><<<grid, THREADS, 0, s>>>(a, (float*)out);
        else slot_vis_grid_kernel<float, 0><<<grid, THREADS, 0, s>>>(a, (float*)out);
    }
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
