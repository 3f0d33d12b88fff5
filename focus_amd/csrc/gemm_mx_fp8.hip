// gemm_mx_fp8.hip -- MX-scaled fp8 NT GEMM:  C[M,N] = epi(alpha * w_scale * sum_k A[m,k] 2^e[m,k/32] . W[n,k] + bias) [+ res]
// with A the e4m3 codes of the activations and one E8M0 scale per 32 elements of a row (mx_quant.hip), W the e4m3 codes
// of the weights with ONE fp32 scale per tensor (fp8.hip), bf16 out.
//
// Why: the fp8-weight instance of gemm_mfma_ws.hip widens the weight codes to bf16 and runs the bf16 MFMA, so the A
// operand still fills the LDS ring at 128 bytes per row for 64 elements of K, and the MFMA rate stays the bf16 rate.  With
// both operands in e4m3 a K-step of 128 elements is the SAME 128-byte row stage for A and for B: half the LDS-fill bytes
// per flop on both operands, and v_mfma_scale_f32_16x16x128_f8f6f4 runs at twice the bf16 rate per clock
// (MI355X_MICROARCH.md, fp8 row).  The structure is that of gemm_mfma_ws.hip: a persistent 768-thread workgroup, 8
// consumer waves (ds_read_b128 + the scaled MFMA only) and 4 loader waves (global_load_lds only) running two K-steps ahead
// through a 3-stage LDS ring, one raw s_barrier per K-step, XCD-banded tile order, and the same bf16 epilogue through
// per-wave LDS slabs (tile shapes: focus_gemm_mx below).
//
// Operand maps of the scaled 16x16x128 instruction with e4m3 operands (measured on the MI355X with one-hot codes and a
// distinct scale per lane; tests/test_gpu_fp8_act.py checks them with exact integer data): lane l = 16 g + c holds row /
// column c, bytes 0-15 = k 16 g .. +15 and bytes 16-31 = k 64 + 16 g .. +15, i.e. the 16-byte chunks g and g + 4 of a
// 128-byte LDS row; the scale byte passed by lane group g covers the 32-element block g (k 32 g .. +31), which lane groups
// 2 (g & 1) and 2 (g & 1) + 1 hold in their low (g < 2) or high (g >= 2) halves.  So lane group g passes the scale of block
// g of its row, whichever codes it holds itself.
// As in gemm_mfma_ws.hip the weight fragment is the instruction's FIRST operand (C/D row = output column n, C/D column =
// output row m), so the activation scale goes in the SECOND scale slot; the weights' slot holds 127 (2^0) in every byte.
// The activation scales of a K-step (4 bytes per row) ride the ring: each loader wave adds one 4-byte-per-lane LDS-DMA
// piece (64 rows) per K-step, so the consumers never issue a global load and every wait stays a counted one.
#include "focus_common.h"
#include "gemm_internal.h"
#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

constexpr int BK = 128;                       // elements (= bytes) of K per ring stage and per MFMA
constexpr int W_SCALE = 0x7f7f7f7f;           // E8M0 127 = 2^0 in every byte: the weights carry their scale in the epilogue

__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

struct Unit { int m0, n0; };

// Consumer grid WM x WN waves, each a (16 MI) x 64 output tile.  NLOAD loader waves; A_BYTES + B_BYTES + the activation
// scales of NLOAD x 64 rows per stage.
template <int WM, int WN, int MI, int EPI, int NLOAD, int NSTAGE>
__global__ __launch_bounds__(64 * (WM * WN + NLOAD)) void gemm_mx_kernel(const focus_gemm_desc d, const uint8_t* __restrict__ as,
                                                                          int64_t ld_as, int tiles_m, int tiles_n, int GM) {
    constexpr int BM = WM * MI * 16, BN = WN * 64;
    constexpr int NCONS = WM * WN;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES + NLOAD * 256;
    constexpr int GA = BM / 8 / NLOAD, GB = BN * 128 / 1024 / NLOAD;   // 1 KiB DMA pieces per loader wave per K-step
    static_assert(GA * 8 * NLOAD == BM && GB * 1024 * NLOAD == BN * 128, "pieces must divide among the loader waves");
    static_assert(NLOAD * 64 >= BM, "one scale piece per loader wave must cover the tile's rows");
    constexpr int PIECES = GA + GB + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint8_t* A = static_cast<const uint8_t*>(d.A);
    const uint8_t* B = static_cast<const uint8_t*>(d.B);
    bf16_t* C = static_cast<bf16_t*>(d.C);
    const bf16_t* R = static_cast<const bf16_t*>(d.residual);
    bf16_t* X = static_cast<bf16_t*>(d.aux);
    const int64_t lda = d.rsA, ldb = d.csB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- unit schedule (identical for both roles): XCD-banded, round-robin inside the band (gemm_mfma_ws.hip) ----
    const int nunits = tiles_m * tiles_n, nk = d.K / BK;
    const int G = gridDim.x, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int gx = (G >> 3) + (xcd < (G & 7) ? 1 : 0);
    const int q = nunits >> 3, r = nunits & 7;
    const int band0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int band_n = q + (xcd < r ? 1 : 0);
    const int my_units = j < band_n ? (band_n - j + gx - 1) / gx : 0;
    if (my_units == 0) return;
    auto unit_of = [&](int i) __attribute__((always_inline)) {
        const int u = band0 + j + i * gx;
        const int group = u / (GM * tiles_n), first_m = group * GM;
        const int gsz = min(tiles_m - first_m, GM), in_g = u - group * GM * tiles_n;
        Unit t;
        t.m0 = (first_m + in_g % gsz) * BM;
        t.n0 = (in_g / gsz) * BN;
        return t;
    };
    const int total = my_units * nk;

    if (w >= NCONS) {
        // =============================== loader waves ===============================
        const int L = w - NCONS;
        const int lrow = lane >> 3, csrc = ((lane & 7) ^ lrow) * 16;    // row of a 1 KiB piece, pre-swizzled source chunk
        const uint8_t* a_src[GA];
        const uint8_t* b_src[GB];
        const uint8_t* s_src;
        int iu = 0, ikt = 0;
        auto setup = [&](int i) __attribute__((always_inline)) {
            const Unit t = unit_of(i);
#pragma unroll
            for (int g = 0; g < GA; ++g) a_src[g] = A + (int64_t)min(t.m0 + (L * GA + g) * 8 + lrow, d.M - 1) * lda + csrc;
#pragma unroll
            for (int g = 0; g < GB; ++g) b_src[g] = B + (int64_t)min(t.n0 + (L * GB + g) * 8 + lrow, d.N - 1) * ldb + csrc;
            s_src = as + (int64_t)min(t.m0 + L * 64 + lane, d.M - 1) * ld_as;   // rows past the tile: loaded, never read
        };
        auto issue = [&](int st) __attribute__((always_inline)) {
            char* sa = smem + st * STAGE;
            char* sb = sa + A_BYTES;
            char* ss = sb + B_BYTES;
#pragma unroll
            for (int g = 0; g < GA; ++g)
                __builtin_amdgcn_global_load_lds((gvoid_t*)(a_src[g] + ikt * BK), (lvoid_t*)(sa + (L * GA + g) * 1024), 16, 0, 0);
#pragma unroll
            for (int g = 0; g < GB; ++g)
                __builtin_amdgcn_global_load_lds((gvoid_t*)(b_src[g] + ikt * BK), (lvoid_t*)(sb + (L * GB + g) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvoid_t*)(s_src + ikt * 4), (lvoid_t*)(ss + L * 256), 4, 0, 0);
            if (++ikt == nk) { ikt = 0; if (++iu < my_units) setup(iu); }
        };
        constexpr int AHEAD = NSTAGE - 1;
        constexpr int INFLIGHT = (AHEAD - 1) * PIECES;
        setup(0);
        issue(0);
        if (AHEAD > 1 && total >= AHEAD) {
#pragma unroll
            for (int a = 1; a < AHEAD; ++a) issue(a);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT) : "memory");
        } else {
            for (int a = 1; a < AHEAD && a < total; ++a) issue(a);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                      // step 0 is in LDS
        int st2 = AHEAD % NSTAGE, ckt = 0;
        for (int t = 0; t < total; ++t) {
            if (t + AHEAD < total) {
                issue(st2);
                st2 = st2 == NSTAGE - 1 ? 0 : st2 + 1;
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT) : "memory");   // step t+1 landed, later steps in flight
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();                  // end of K-step t
            if (++ckt == nk) {
                ckt = 0;
                __builtin_amdgcn_s_barrier();              // barrier E (epilogue done, stage reusable)
            }
        }
        return;
    }

    // =============================== consumer waves ===============================
    const int wm = w / WN, wn = w % WN;
    const int frow = lane & 15, fq = lane >> 4;
    const float alpha = d.alpha * *d.b_scale;
    f32x4 acc[MI][4];
    auto frag = [&](const char* s, int row) __attribute__((always_inline)) {
        // the codes k = 16 fq .. +15 and 64 + 16 fq .. +15 of `row`: chunks fq and fq + 4, one ds_read_b128 each
        const uint4 lo = *reinterpret_cast<const uint4*>(s + swz(row, fq));
        const uint4 hi = *reinterpret_cast<const uint4*>(s + swz(row, fq + 4));
        return (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    };
    auto compute = [&](const char* sa) __attribute__((always_inline)) {
        const char* sb = sa + A_BYTES;
        const uint8_t* ss = reinterpret_cast<const uint8_t*>(sb + B_BYTES);
        i32x8 fb[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) fb[jj] = frag(sb, wn * 64 + jj * 16 + frow);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int row = wm * (16 * MI) + i * 16 + frow;
            const i32x8 fa = frag(sa, row);
            const int sc = ss[row * 4 + fq];               // E8M0 of (row, 32-element block fq of this K-step)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                acc[i][jj] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[jj], fa, acc[i][jj], 0, 0, 0, W_SCALE, 0, sc);
        }
    };
    auto epilogue = [&](char* stage, int m0, int n0) __attribute__((always_inline)) {
        // as gemm_mfma_ws.hip: the wave's tile leaves in 32-row halves through a private 4 KiB slab
        // ([32 rows][16 chunks of 8 B], chunk ^= row & 15) inside the just-consumed stage
        char* slab = stage + w * 4096;
#pragma unroll
        for (int half = 0; half < (MI + 1) / 2; ++half) {
            constexpr int LASTN = (MI & 1) ? 1 : 2;
            const int nfr = (half == (MI + 1) / 2 - 1) ? LASTN : 2;
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2) {
                if (i2 >= nfr) break;
                const int i = half * 2 + i2, row = i2 * 16 + frow;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int gn = n0 + wn * 64 + jj * 16 + fq * 4;
                    float t[4];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        t[r4] = alpha * acc[i][jj][r4];
                        if (d.bias && gn + r4 < d.N) t[r4] += d.bias[gn + r4];
                    }
                    uint2 pk;
                    pk.x = (uint32_t)f32_to_bf16(t[0]) | ((uint32_t)f32_to_bf16(t[1]) << 16);
                    pk.y = (uint32_t)f32_to_bf16(t[2]) | ((uint32_t)f32_to_bf16(t[3]) << 16);
                    *reinterpret_cast<uint2*>(slab + row * 128 + (((jj * 4 + fq) ^ (row & 15)) << 3)) = pk;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int q8 = lane & 7;
#pragma unroll
            for (int p8 = 0; p8 < 4; ++p8) {
                if (p8 >= 2 * nfr) break;
                const int row = p8 * 8 + (lane >> 3);
                const int gm = m0 + wm * (16 * MI) + half * 32 + row, gn = n0 + wn * 64 + q8 * 8;
                uint4 raw = *reinterpret_cast<const uint4*>(slab + row * 128 + ((q8 ^ ((row & 15) >> 1)) << 4));
                if (row & 1) { const uint32_t a0 = raw.x, a1 = raw.y; raw.x = raw.z; raw.y = raw.w; raw.z = a0; raw.w = a1; }
                if (gm >= d.M || gn >= d.N) continue;
                const int64_t off = gm * d.rsC + gn;
                float v[8] = {__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u),
                              __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u),
                              __uint_as_float(raw.z << 16), __uint_as_float(raw.z & 0xffff0000u),
                              __uint_as_float(raw.w << 16), __uint_as_float(raw.w & 0xffff0000u)};
                if constexpr (EPI == FOCUS_EPI_GELU) { if (X) *reinterpret_cast<uint4*>(X + off) = raw; }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if constexpr (EPI == FOCUS_EPI_GELU) v[e] = gelu_erf(v[e]);
                    else if constexpr (EPI == FOCUS_EPI_RELU) v[e] = fmaxf(v[e], 0.f);
                }
                if (R) {
                    const uint4 rr = *reinterpret_cast<const uint4*>(R + off);
                    v[0] += __uint_as_float(rr.x << 16); v[1] += __uint_as_float(rr.x & 0xffff0000u);
                    v[2] += __uint_as_float(rr.y << 16); v[3] += __uint_as_float(rr.y & 0xffff0000u);
                    v[4] += __uint_as_float(rr.z << 16); v[5] += __uint_as_float(rr.z & 0xffff0000u);
                    v[6] += __uint_as_float(rr.w << 16); v[7] += __uint_as_float(rr.w & 0xffff0000u);
                }
                uint4 o;
                o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
                o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
                o.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
                o.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
                typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
                __builtin_nontemporal_store((u32x4){o.x, o.y, o.z, o.w}, reinterpret_cast<u32x4*>(C + off));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // slab re-read before the second half overwrites it
        }
    };

    __builtin_amdgcn_s_barrier();                          // step 0 is in LDS
    int st = 0;
    for (int cu = 0; cu < my_units; ++cu) {
        const Unit cur = unit_of(cu);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        char* last_stage = smem;
        for (int kt = 0; kt < nk; ++kt) {
            char* sa = smem + st * STAGE;
            compute(sa);
            last_stage = sa;
            st = st == NSTAGE - 1 ? 0 : st + 1;
            __builtin_amdgcn_s_barrier();                  // end of this K-step (every consumer is done with `sa`)
        }
        epilogue(last_stage, cur.m0, cur.n0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // barrier E
    }
}

template <int WM, int WN, int MI, int EPI>
int launch_mx(const focus_gemm_desc& d, const uint8_t* as, int64_t ld_as, hipStream_t s) {
    constexpr int NLOAD = 4, BM = WM * MI * 16, BN = WN * 64;
    constexpr int STAGE = BM * 128 + BN * 128 + NLOAD * 256;
    constexpr int FIT = 160 * 1024 / STAGE;
    constexpr int NSTAGE = FIT >= 4 ? 4 : FIT;
    static_assert(NSTAGE >= 3, "the loaders run two K-steps ahead");
    const int tiles_m = (d.M + BM - 1) / BM, tiles_n = (d.N + BN - 1) / BN;
    const size_t lds = (size_t)NSTAGE * STAGE;
    auto k = gemm_mx_kernel<WM, WN, MI, EPI, NLOAD, NSTAGE>;
    static bool once = (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess);
    (void)once;
    const int nunits = tiles_m * tiles_n;
    dim3 grid(std::min(nunits, 256), 1);
    const int gm = tiles_n <= 4 ? 1 : 8;                   // as gemm_mfma_ws.hip: narrow outputs walk a row of tiles first
    hipLaunchKernelGGL(k, grid, dim3(64 * (WM * WN + NLOAD)), lds, s, d, as, ld_as, tiles_m, tiles_n, gm);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

template <int WM, int WN, int MI>
int launch_mx_epi(const focus_gemm_desc& d, const uint8_t* as, int64_t ld_as, hipStream_t s) {
    switch (d.epilogue) {
        case FOCUS_EPI_NONE: return launch_mx<WM, WN, MI, FOCUS_EPI_NONE>(d, as, ld_as, s);
        case FOCUS_EPI_GELU: return launch_mx<WM, WN, MI, FOCUS_EPI_GELU>(d, as, ld_as, s);
        case FOCUS_EPI_RELU: return launch_mx<WM, WN, MI, FOCUS_EPI_RELU>(d, as, ld_as, s);
        default: return FOCUS_ERR_SHAPE;
    }
}

}  // namespace

extern "C" int focus_gemm_mx(const focus_gemm_desc* desc, const void* a_scales, int64_t ld_a_scales, void* stream) {
    if (!desc || !desc->A || !desc->B || !desc->C || !a_scales || !desc->b_scale) return FOCUS_ERR_NULL;
    focus_gemm_desc d = *desc;
    if (d.batch0 < 1) d.batch0 = 1;
    if (d.batch1 < 1) d.batch1 = 1;
    if (d.dtype_ab != FOCUS_FP8_E4M3 || d.dtype_b != FOCUS_FP8_E4M3 || d.dtype_c != FOCUS_BF16 || d.accumulate)
        return FOCUS_ERR_DTYPE;
    if (d.batch0 * d.batch1 != 1 || d.M < 0 || d.N <= 0 || (d.N % 64) != 0 || d.K <= 0 || (d.K % BK) != 0)
        return FOCUS_ERR_SHAPE;
    if (d.epilogue != FOCUS_EPI_NONE && d.epilogue != FOCUS_EPI_GELU && d.epilogue != FOCUS_EPI_RELU) return FOCUS_ERR_SHAPE;
    if (d.csA != 1 || d.rsB != 1 || d.csC != 1 || d.rsA < d.K || d.csB < d.K || d.rsC < d.N || ld_a_scales < d.K / 32)
        return FOCUS_ERR_SHAPE;
    if (!focus_aligned(d.A, 16) || !focus_aligned(d.B, 16) || !focus_aligned(d.C, 16) || (d.rsA & 15) || (d.csB & 15) ||
        (d.rsC & 7) || !focus_aligned(a_scales, 4) || (ld_a_scales & 3) || !focus_aligned(d.b_scale, 4) ||
        (d.residual && !focus_aligned(d.residual, 16)) || (d.aux && !focus_aligned(d.aux, 16)))
        return FOCUS_ERR_ALIGN;
    if (d.epilogue != FOCUS_EPI_GELU) d.aux = nullptr;
    if (d.M == 0) return FOCUS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* as = static_cast<const uint8_t*>(a_scales);
    focus_gemm_note_kernel(FOCUS_GEMM_KERNEL_NT_MX);
    // 128 x 256 tiles; narrow outputs (N = 64 .. 192) 256 x 128.  The 160-row tile of gemm_mfma_ws.hip is not built here:
    // with 32-byte fragments it needs 168 VGPRs at 3 waves per SIMD and spills; by the modelled rounds of the 256 CUs
    // (rows per tile + ~40 rows of fixed cost) it would win none of the HR shapes but 14116 x 3072 (by 1 %)
    if (d.N >= 256) return launch_mx_epi<2, 4, 4>(d, as, ld_a_scales, s);
    return launch_mx_epi<4, 2, 4>(d, as, ld_a_scales, s);   // N = 64 .. 192: 256 x 128 tiles
}
