"""TEST INFRASTRUCTURE: CPU twin of csrc/random_erase.hip and the cases of tests/golden/random_erasing.npz
(tests/make_random_erasing_golden.py).

Planner.  `plan` restates what RandomErasing draws from Python's `random` and which rectangles follow, from the reference's
description alone: the gate, the count, per rectangle the attempts of two uniforms and on a fit two randints.

Fill values.  `hashes` restates the generator of include/focus_amd.h in numpy integers, `normals` turns them into the
Box-Muller value in fp64, `normals_f32` restates the kernel's fp32 arithmetic (with switches for the mutants the tests
run).  With ha, hb the two hashed words of a position word (in mode "pixel" columns 2m and 2m + 1 of a row share the word
(y << 16) | m; the even column takes the cosine, the odd one the sine: the two independent values of one draw):
    u1 = ((ha >> 9) + 1/2) / 2^23,   u2 = (hb >> 8) / 2^24,   z = sqrt(-2 ln u1) cos(2 pi u2)  or  sqrt(-2 ln u1) sin(2 pi u2).

BOUND between the kernel's fp32 z and the fp64 value, term by term (ulp limits of the device library: the OpenCL
single-precision limits it is built to, log 3 ulp, sqrt 3 ulp, cospi and sinpi 4 ulp):
  * the uniform: (ha >> 9) + 1/2 is a 24-bit number and 2^-23 a power of two, so u1 is EXACT in fp32; likewise the angle,
    which reaches sincospif as 2 u2 = (hb >> 8) / 2^23 half turns and is never multiplied by a rounded pi: EXACT;
  * L = logf(u1): 3 ulp, a relative error of at most 3 * 2^-23 (an ulp is at most 2^-23 of its value); -2 L is exact;
  * r = sqrtf(-2 L): half the relative error of its argument, 3 * 2^-24, plus its own 3 ulp <= 6 * 2^-24;
  * cospif / sinpif: 4 ulp of a value of at most 1: an absolute error of at most 4 * 2^-24;
  * the product r * cos (or r * sin): one rounding, a relative error of at most 2^-24 of |z| <= r.
  |dz| <= r (3 + 6) 2^-24 |cos| + r 4 * 2^-24 + r 2^-24 <= R_MAX * 14 * 2^-24 = 4.82e-6, with the largest reachable
  r = |z| = R_MAX = sqrt(2 ln 2^24) = 5.768 (u1 >= 2^-24); second-order terms are below 1e-12.
bf16 output adds one round-to-nearest-even of the fp32 value: half a bf16 ulp of the value (bf16_half_ulp)."""
import math
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_erasing.npz")

T, C, H, W = 4, 3, 10, 14          # the fixture's clip [T,C,H,W] and image [C,H,W]

E_LOG, E_SQRT, E_COS = 3, 3, 4
R_MAX = math.sqrt(2.0 * math.log(2.0 ** 24))
BOUND = R_MAX * (E_LOG + 2 * E_SQRT + E_COS + 1) * 2.0 ** -24

# name -> (RandomErasing keyword arguments, input: "clip", "view" (the permuted [C,T,H,W] clip of ssv2.py:444) or "image",
#          what the seed search looks for)
CASES = {
    "gate_closed":   (dict(probability=0.25, mode="pixel", max_count=1, num_splits=1), "clip", "closed"),
    "one_const":     (dict(probability=0.25, mode="const", max_count=1, num_splits=1), "clip", "one"),
    "one_rand":      (dict(probability=0.25, mode="rand", max_count=1, num_splits=1), "view", "one"),
    "one_pixel":     (dict(probability=0.25, mode="pixel", max_count=1, num_splits=1), "view", "one"),
    "retry":         (dict(probability=0.5, mode="rand", max_count=1, num_splits=1), "clip", "retry"),
    "count2_clean":  (dict(probability=0.5, mode="const", max_count=2, num_splits=2), "clip", "two"),
    "count3_overlap": (dict(probability=0.5, mode="pixel", max_count=3, num_splits=3), "clip", "overlap"),
    "per_frame":     (dict(probability=0.5, mode="rand", max_count=2, num_splits=0, cube=False), "clip", "frames"),
    "image":         (dict(probability=0.5, mode="pixel"), "image", "one"),
}


def fixture():
    return np.load(GOLDEN, allow_pickle=False)


# ---- the planner ---------------------------------------------------------------------------------------------------
def _rectangles(probability, lo_area, hi_area, log_lo, log_hi, min_count, max_count, frame_h, frame_w, tries):
    """One gate and what follows it -> [(top, left, h, w)], and the number of attempts each rectangle took."""
    if random.random() > probability:
        return [], []
    n = min_count if min_count == max_count else random.randint(min_count, max_count)
    rects, attempts = [], []
    for _ in range(n):
        for k in range(tries):
            share = random.uniform(lo_area, hi_area) * (frame_h * frame_w) / n
            ratio = math.exp(random.uniform(log_lo, log_hi))
            h, w = int(round(math.sqrt(share * ratio))), int(round(math.sqrt(share / ratio)))
            if w < frame_w and h < frame_h:
                top = random.randint(0, frame_h - h)
                rects.append((top, random.randint(0, frame_w - w), h, w))
                attempts.append(k + 1)
                break
    return rects, attempts


def plan(kw, n, frame_h, frame_w, with_attempts=False):
    """kw: RandomErasing keyword arguments; n frames (None: an image) -> int64 [k, 6] rows (t0, t1, top, left, h, w) in the
    order they are written.  Consumes Python's `random`."""
    min_aspect = kw.get("min_aspect", 0.3)
    max_aspect = kw.get("max_aspect") or 1 / min_aspect
    min_count = kw.get("min_count", 1)
    args = (kw.get("probability", 0.5), kw.get("min_area", 0.02), kw.get("max_area", 1 / 3), math.log(min_aspect),
            math.log(max_aspect), min_count, kw.get("max_count") or min_count, frame_h, frame_w)
    rows, tries = [], []
    if n is None:
        spans = [((0, 1), 10)]
    else:
        splits = kw.get("num_splits", 0)
        first = n // splits if splits > 1 else 0
        spans = [((first, n), 100)] if kw.get("cube", True) else [((i, i + 1), 10) for i in range(first, n)]
    for (t0, t1), limit in spans:
        rects, attempts = _rectangles(*args, limit)
        rows += [(t0, t1) + r for r in rects]
        tries += attempts
    rows = np.array(rows, dtype=np.int64).reshape(-1, 6)
    return (rows, tries) if with_attempts else rows


def overlaps(rows):
    """True when two rows share a frame and a pixel."""
    for i, a in enumerate(rows):
        for b in rows[i + 1:]:
            if max(a[0], b[0]) < min(a[1], b[1]) and max(a[2], b[2]) < min(a[2] + a[4], b[2] + b[4]) and \
                    max(a[3], b[3]) < min(a[3] + a[5], b[3] + b[5]):
                return True
    return False


# ---- the generator -------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xffffffff)
_G = np.uint64(0x9E3779B9)
FLAT = 0xffffffff                  # the position word of the one value per (item, frame, channel) of mode "rand"


def _u64(v):
    return np.asarray(v).astype(np.int64).astype(np.uint64) & _M32      # negative int32 words wrap


def mix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _M32
    x ^= x >> np.uint64(16)
    return x


def hashes(s0, s1, ord_, clip, t, c, p):
    """The two hashed words (ha, hb) of position word p under (seed, item ordinal, clip, frame, channel); arguments
    broadcast."""
    h = mix32(_u64(s0) ^ _u64(clip))
    h = mix32((h + _u64(ord_) * _G) & _M32)
    h = mix32(h ^ _u64(t))
    key = mix32((h + _u64(c) * _G) & _M32)
    ha = mix32(key ^ _u64(p))
    return ha, mix32(ha ^ _u64(s1))


def position(y, x):
    """The position word of element (y, x) in mode "pixel": the row and the column PAIR."""
    return (_u64(y) << np.uint64(16)) | (_u64(x) >> np.uint64(1))


def normals(ha, hb, odd=False):
    """fp64 Box-Muller value of the hashed words: the cosine branch, or the sine branch where `odd` (an odd column)."""
    u1 = ((ha >> np.uint64(9)).astype(np.float64) + 0.5) / 2.0 ** 23
    angle = 2.0 * np.pi * ((hb >> np.uint64(8)).astype(np.float64) / 2.0 ** 24)
    return np.sqrt(-2.0 * np.log(u1)) * np.where(odd, np.sin(angle), np.cos(angle))


def normals_f32(ha, hb, odd=False, sine=False, drop_half=False):
    """The kernel's formula in fp32 operations: exact u1 and angle, logf, sqrtf, sincospif (an exact reduction of the half
    turns to [-1/4, 1/4], then cos or sin of pi f).  sine (the two branches swapped) / drop_half: the mutants."""
    f = np.float32
    u1 = ((ha >> np.uint64(9)).astype(f) + f(0.0 if drop_half else 0.5)) * f(2.0 ** -23)
    with np.errstate(divide="ignore"):
        r = np.sqrt(f(-2.0) * np.log(u1)).astype(f)
    turns = (hb >> np.uint64(8)).astype(f) * f(2.0 ** -23)                 # [0, 2), exact
    turns = np.where(np.asarray(odd) != sine, turns - f(0.5), turns).astype(f)     # sin(a) = cos(a - pi/2): [-1/2, 3/2), exact
    n = np.rint(turns * f(2.0))
    frac = (turns - n * f(0.5)).astype(f)                                   # exact
    arg = (f(np.pi) * frac).astype(f)
    q = n.astype(np.int64) % 4
    cs, sn = np.cos(arg).astype(f), np.sin(arg).astype(f)
    trig = np.where(q == 0, cs, np.where(q == 1, -sn, np.where(q == 2, -cs, sn))).astype(f)
    return (r * trig).astype(f)


def bf16_half_ulp(v):
    """Half a bf16 ulp of each value (8 significant bits)."""
    _m, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 8 - 1))


def table(items):
    """[(clip, t0, t1, top, left, h, w)] -> int32 [n, 8] rows with `ord`, the clips' items contiguous in listing order."""
    rows, seen = [], {}
    for it in items:
        k = seen.get(it[0], 0)
        rows.append(tuple(it) + (k,))
        seen[it[0]] = k + 1
    rows.sort(key=lambda r: (r[0], r[7]))
    return np.array(rows, dtype=np.int32).reshape(-1, 8)


def expected(shape, rows, mode, s0, s1):
    """What the launch leaves in a LOGICAL [B,C,T,H,W] tensor: (written mask, fp64 values, owner: the table row that
    wrote each element or -1).  rows: `table`'s; applied in order, so the last item of a clip that covers an element wins."""
    written, vals, owner = np.zeros(shape, bool), np.zeros(shape), np.full(shape, -1)
    for k, (clip, t0, t1, top, left, h, w, ord_) in enumerate(np.asarray(rows).tolist()):
        sl = (clip, slice(None), slice(t0, t1), slice(top, top + h), slice(left, left + w))
        cc, tt, yy, xx = np.meshgrid(np.arange(shape[1]), np.arange(t0, t1), np.arange(top, top + h),
                                     np.arange(left, left + w), indexing="ij")
        if mode == "const":
            z = np.zeros(cc.shape)
        else:
            z = normals(*hashes(s0, s1, ord_, clip, tt, cc, position(yy, xx) if mode == "pixel" else FLAT),
                        odd=(xx & 1) == 1 if mode == "pixel" else False)
        written[sl], vals[sl], owner[sl] = True, z, k
    return written, vals, owner
