// random_erase.hip -- RandomErasing of a batch of normalised clips in place, in one launch (datasets/random_erasing.py of the
// reference: the last step of Ssv2._aug_frame, ssv2.py:436-446).  The host plans the rectangles with the reference's draws
// (slowfast/datasets/random_erasing.py here); this file writes them.
//
// Work split: blockIdx.y is the item, so the descriptor is block-uniform.  A thread owns one 16-byte-aligned chunk (4 fp32 or
// 8 bf16) of one row of the rectangle in one channel of one frame; the threads of an item stride over its chunks, so any grid
// gives the same result.  A chunk the rectangle covers entirely is one 16-byte store; the chunks its left and right edges
// cut are written element by element.  Nothing is loaded from the tensor.
//
// Overlap: the reference writes the rectangles of a clip one after another, so the last one wins.  Here the owner of a chunk
// of item i scans the items behind i (at most max_per_clip - 1 of them, those of the same clip) and masks out the elements
// one of them covers: every element is written by exactly one thread, whatever the order the workgroups run in.
//
// Draws: a value is a hash of (seed, item ordinal, clip, frame, channel, y, x) in the tensor's LOGICAL coordinates, pushed
// through Box-Muller; the formula is stated in include/focus_amd.h and restated in numpy in tests/erase_ref.py.  The uniform
// and the angle are exact fp32 numbers (sincospif takes the angle in half turns: no product with pi is rounded), and logf,
// sqrtf and sincospif are the accurate library versions, so the bound the tests hold the values to follows from published
// ulp limits.  That arithmetic, not memory, is what the kernel's time goes to (profiles/erase_bench.txt); a pair of
// neighbouring columns shares one Box-Muller draw (its cosine and its sine), which halves it.
#include "focus_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS_X = 256;    // per item; the loop strides over the rest
constexpr int TRIPS = 4;
constexpr uint32_t kGolden = 0x9E3779B9u;

// lowbias32, the finaliser of the build-owned generators (gumbel.hip holds the same function)
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// Box-Muller on the two hashed words of position word p under the (seed, item, clip, frame, channel) key: the radius and the
// sine and cosine of the angle, i.e. TWO independent N(0,1) values, r * c and r * s
struct Polar { float r, s, c; };
__device__ __forceinline__ Polar polar_draw(uint32_t key, uint32_t p, uint32_t s1) {
    const uint32_t ha = mix32(key ^ p), hb = mix32(ha ^ s1);
    const float u1 = ((float)(ha >> 9) + 0.5f) * (1.0f / 8388608.0f);      // (k + 1/2) / 2^23: 24 bits, exact
    const float turns = (float)(hb >> 8) * (1.0f / 8388608.0f);            // 2 u2 in [0, 2): the angle in half turns, exact
    Polar d;
    d.r = sqrtf(-2.0f * logf(u1));
    sincospif(turns, &d.s, &d.c);
    return d;
}
// mode "pixel": columns 2m and 2m + 1 of a row share the draw of position word (y << 16) | m, the even one takes the
// cosine.  `d` holds the draw of column col - 1's pair on entry when `have`; returns the value of column col.
__device__ __forceinline__ float pixel_value(Polar& d, bool have, uint32_t key, int y, int col, uint32_t s1) {
    if (!have || !(col & 1)) d = polar_draw(key, ((uint32_t)y << 16) | (uint32_t)(col >> 1), s1);
    return (col & 1) ? d.r * d.s : d.r * d.c;
}

// an item clamped to the tensor: frames [t0,t1), rows [y0,y1), columns [x0,x1); empty() when nothing is left
struct Box {
    int t0, t1, y0, y1, x0, x1;
    __device__ __forceinline__ bool empty() const { return t0 >= t1 || y0 >= y1 || x0 >= x1; }
};
__device__ __forceinline__ Box clamp_item(const focus_erase_item& it, int T, int H, int W) {
    Box b;
    b.t0 = max(it.t0, 0);
    b.t1 = min(it.t1, T);
    b.y0 = max(it.top, 0);
    b.y1 = (int)min((int64_t)it.top + max(it.h, 0), (int64_t)H);
    b.x0 = max(it.left, 0);
    b.x1 = (int)min((int64_t)it.left + max(it.w, 0), (int64_t)W);
    return b;
}

template <typename T, int VEC> __device__ __forceinline__ void store_chunk(T* p, const float (&v)[VEC]);
template <> __device__ __forceinline__ void store_chunk<float, 4>(float* p, const float (&v)[4]) {
    st4<float>(p, {v[0], v[1], v[2], v[3]});
}
template <> __device__ __forceinline__ void store_chunk<bf16_t, 8>(bf16_t* p, const float (&v)[8]) { st8<bf16_t>(p, v); }

template <typename T, int MODE>
__global__ __launch_bounds__(THREADS) void random_erase_kernel(T* __restrict__ x, int B, int nT, int C, int H, int W, int64_t sb,
                                                               int64_t sc, int64_t st_, const focus_erase_item* __restrict__ items,
                                                               int n_items, int max_per_clip, const uint32_t* __restrict__ seed) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int i = blockIdx.y;
    const focus_erase_item it = items[i];
    const Box r = clamp_item(it, nT, H, W);
    if (it.clip < 0 || it.clip >= B || r.empty()) return;
    const int last = min(n_items - 1, i + max_per_clip - 1);          // the items behind i that may belong to its clip
    const int h = r.y1 - r.y0, w = r.x1 - r.x0;
    const int nchunk = (w + VEC - 1) / VEC + 1;                        // aligned chunks a row of w elements can touch
    const int64_t units = (int64_t)(r.t1 - r.t0) * C * h * nchunk;
    uint32_t s1 = 0, item_key = 0;
    if (MODE != FOCUS_ERASE_CONST) {
        s1 = seed[1];
        item_key = mix32(mix32(seed[0] ^ (uint32_t)it.clip) + (uint32_t)it.ord * kGolden);
    }
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t u = (int64_t)blockIdx.x * THREADS + threadIdx.x; u < units; u += stride) {
        int64_t q = u / nchunk;
        const int j = (int)(u - q * nchunk);
        const int y = r.y0 + (int)(q % h);
        q /= h;
        const int c = (int)(q % C), t = r.t0 + (int)(q / C);
        T* row = x + (int64_t)it.clip * sb + (int64_t)c * sc + (int64_t)t * st_ + (int64_t)y * W;
        // chunk j holds the columns [lo, lo + VEC); row + lo is 16-byte aligned (a: how far column x0 is past such an address)
        const int a = (int)((reinterpret_cast<uintptr_t>(row + r.x0) / sizeof(T)) & (uintptr_t)(VEC - 1));
        const int lo = r.x0 - a + j * VEC, hi = lo + VEC;
        const int xs = max(lo, r.x0), xe = min(hi, r.x1);
        if (xs >= xe) continue;
        uint32_t skip = 0;                                             // bit e: column lo + e belongs to a later item
        for (int k = i + 1; k <= last; ++k) {
            const focus_erase_item o = items[k];
            if (o.clip != it.clip) break;
            const Box ob = clamp_item(o, nT, H, W);
            if (ob.empty() || t < ob.t0 || t >= ob.t1 || y < ob.y0 || y >= ob.y1) continue;
            const int cs = max(ob.x0, xs) - lo, ce = min(ob.x1, xe) - lo;
            if (cs < ce) skip |= ((1u << (ce - cs)) - 1u) << cs;     // ce - cs <= VEC <= 8
        }
        uint32_t key = 0;
        float flat = 0.0f;
        if (MODE != FOCUS_ERASE_CONST) key = mix32(mix32(item_key ^ (uint32_t)t) + (uint32_t)c * kGolden);
        Polar d = {0.0f, 0.0f, 0.0f};
        if (MODE == FOCUS_ERASE_RAND) {
            d = polar_draw(key, 0xffffffffu, s1);
            flat = d.r * d.c;
        }
        if (xs == lo && xe == hi && skip == 0) {
            float v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = MODE == FOCUS_ERASE_PIXEL ? pixel_value(d, e > 0, key, y, lo + e, s1) : flat;
            store_chunk<T, VEC>(row + lo, v);
        } else {
            for (int col = xs; col < xe; ++col) {
                const float v = MODE == FOCUS_ERASE_PIXEL ? pixel_value(d, col > xs, key, y, col, s1) : flat;
                if (!((skip >> (col - lo)) & 1u)) st<T>(row + col, v);
            }
        }
    }
}

template <typename T>
void launch(int mode, dim3 grid, hipStream_t s, T* x, int B, int nT, int C, int H, int W, int64_t sb, int64_t sc, int64_t st_,
            const focus_erase_item* items, int n_items, int max_per_clip, const uint32_t* seed) {
    if (mode == FOCUS_ERASE_CONST)
        random_erase_kernel<T, FOCUS_ERASE_CONST><<<grid, THREADS, 0, s>>>(x, B, nT, C, H, W, sb, sc, st_, items, n_items, max_per_clip, seed);
    else if (mode == FOCUS_ERASE_RAND)
        random_erase_kernel<T, FOCUS_ERASE_RAND><<<grid, THREADS, 0, s>>>(x, B, nT, C, H, W, sb, sc, st_, items, n_items, max_per_clip, seed);
    else
        random_erase_kernel<T, FOCUS_ERASE_PIXEL><<<grid, THREADS, 0, s>>>(x, B, nT, C, H, W, sb, sc, st_, items, n_items, max_per_clip, seed);
}

}  // namespace

extern "C" int focus_random_erase(void* x, int dtype, int B, int T, int C, int H, int W, int64_t sb, int64_t sc, int64_t st,
                                  const focus_erase_item* items, int n_items, int max_per_clip, int mode, const void* seed,
                                  void* stream) {
    const bool draws = mode == FOCUS_ERASE_RAND || mode == FOCUS_ERASE_PIXEL;
    if (!x || !items || (draws && !seed)) return FOCUS_ERR_NULL;
    if (n_items <= 0) return FOCUS_OK;
    if (!draws && mode != FOCUS_ERASE_CONST) return FOCUS_ERR_SHAPE;
    if (B < 1 || T < 1 || C < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || T > 65535 || C > 65535 || n_items > 65535)
        return FOCUS_ERR_SHAPE;
    if (max_per_clip < 1 || max_per_clip > FOCUS_ERASE_MAX_PER_CLIP) return FOCUS_ERR_SHAPE;
    if (sb < 1 || sc < (int64_t)H * W || st < (int64_t)H * W) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    const size_t es = focus_esize(dtype);
    if (!focus_aligned(x, es)) return FOCUS_ERR_ALIGN;
    // enough threads for a rectangle that fills the frame, capped: smaller rectangles leave some of them without a chunk
    const int64_t units = (int64_t)T * C * H * (W / (int)(16 / es) + 2);
    const int64_t bx = cdiv64(units, (int64_t)THREADS * TRIPS);
    const dim3 grid((unsigned)(bx > MAX_BLOCKS_X ? MAX_BLOCKS_X : bx), (unsigned)n_items);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        launch<bf16_t>(mode, grid, s, (bf16_t*)x, B, T, C, H, W, sb, sc, st, items, n_items, max_per_clip, (const uint32_t*)seed);
    else
        launch<float>(mode, grid, s, (float*)x, B, T, C, H, W, sb, sc, st, items, n_items, max_per_clip, (const uint32_t*)seed);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
