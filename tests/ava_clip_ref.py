"""Reference of the AVA clip kernels (focus_clip_gray_mean / focus_clip_sample_color, include/focus_amd.h): the single-pass
formula in fp64, an fp32 twin in the kernels' order of operations, named wrong variants ("mutants"), and an error bound that
is derived here, not tuned.

    x[c'] = v[c'] / 255                       v: clip_ref.sample's bilinear value of source channel c'
    for the ops of the record, in its order (a = alpha of the op):
        brightness  x = x a;   saturation  x = x a + g (1 - a),  g = sum_c' gray_w[c'] x[c'] of the pixel as it stands
        contrast    x = x a + m_t (1 - a),  m_t = mean of g over the output window of frame t ALONE, as it stands
    x[c'] += shift[c'];   out[c] = (x[c'] - mean[c']) / std[c'],   c' = reverse ? 2-c : c

The bound, per output element, against the fp64 result r (u = 2^-24).  E is the error of x in [0,1] units, M a bound of |x|;
both are carried through the stages.  Roundings are counted for the longer of the reference's order (transform.py:297-517
on fp32 tensors) and the kernels':

  resampling   E = 3 u ((sh + 1) + (sw + 1))  [clip_ref.bound's coordinate term: a full step between neighbouring pixels is
      1 in these units]  +  9 u  [/255, 1-lx, 1-ly, three roundings along x, three along y, at magnitude <= 1; the kernel's two
      lerps and the product with a rounded 1/255 are fewer].  M = 1.
  brightness   E <- |a| E + 2 u |a| M  (a rounded to fp32, the product);  M <- |a| M.
  grey         Eg = E + 8 u M  (weights sum to 1 and are positive; three rounded weights, three products, two sums; the
      kernel's product and two fma are fewer).
  saturation   with G = |a| + |1-a|, the op's gain:  E <- G E + |1-a| 8 u M + 6 u G M  (a and 1-a as fp32 constants -- the
      kernel forms 1-a by an fp32 subtraction from the rounded a: two roundings --, two products, one sum; the kernel's
      product and fma are fewer);  M <- G M.
  contrast     the mean of values with error <= Eg has error <= Eg, plus the summation: additions in a tree of depth D lose
      at most D u max|g| on the mean, one more for the division.  D comes from the order actually implemented (mean_depth:
      8 pixels per thread, 6 butterfly levels, 4 waves, the blocks of a frame in order); for the recorded fp32 frames of the
      reference, whose ATen sum has an order this file does not know, D = 3 h w - 1, the bound of EVERY order of its 3 h w
      terms (any_order=True).  E <- G E + |1-a| (8 + D + 1) u M + 6 u G M;  M <- G M.  The term of the mean is carried
      through the ops after contrast by their gains like everything else in E.
  shift        E <- E + u |s| + u (M + |s|)  (s rounded, the sum);  M <- M + |s|, the largest |s| of the three.
  normalise    per channel (E + 4 u (M + |mean_c|)) / |std_c|  (the kernel: two rounded constants and one fma; the reference:
      a subtraction and a division; one for the store), the largest over the channels.
  bf16 output adds 2^-8 |r|.

A case with scale exactly 1 has no coordinate term (coords=False).

The mutant "listed_order" applies brightness, contrast, saturation as listed and hands them the alphas in the order drawn:
what an implementation that ignores the permutation makes of the same draws.  Moving each op WITH its alpha ("reordered")
is no mutant: all three ops are linear in the frame, brightness is a scalar, and with sum(gray_w) = 1 saturation leaves
every pixel's grey and contrast leaves every frame's mean grey unchanged, so saturation and contrast commute too; the
result differs by roundings only (tests/test_ava_clip_ref_cpu.py holds it inside the bound).  The drawn order matters
through which op receives which draw."""
import os

import numpy as np

import clip_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ava_clip.npz")
U = 2.0 ** -24
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
GRAY_BGR = [0.114, 0.587, 0.299]
MEAN, STD = [0.45, 0.40, 0.35], [0.225, 0.25, 0.2]              # by BGR position; distinct: a wrong channel index shows
EIGVAL = [0.225, 0.224, 0.229]                                   # the reference's defaults (defaults.py:616-624)
EIGVEC = [[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]]
RUN, THREADS = 8, 256

MUTANTS = ("clip_mean", "mean_before_ops", "gray_rgb_position", "pca_same_index", "listed_order", "weights_swapped",
           "norm_first")

# the fixture's cases: tag -> (clip, split, crop size, cfg.AVA overrides); seeds are found by tests/make_ava_clip_golden.py
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
FULL = dict(TRAIN_USE_COLOR_AUGMENTATION=True, TRAIN_PCA_JITTER_ONLY=False)
CASES = {"order%d%d%d" % o: ("ab"[i % 2], "train", (13, 16)[i % 2], dict(FULL, BGR=bool(i % 3 == 0))) for i, o in enumerate(ORDERS)}
CASES.update({
    "pca_only": ("a", "train", 13, dict(TRAIN_USE_COLOR_AUGMENTATION=True, TRAIN_PCA_JITTER_ONLY=True)),
    "no_color": ("b", "train", 16, dict()),
    "val": ("a", "val", 16, dict()),
    "val_flip": ("b", "val", 13, dict(TEST_FORCE_FLIP=True)),
    "val_bgr": ("a", "val", 13, dict(BGR=True)),
})
JITTER = {13: [22, 28], 16: [18, 24]}                            # DATA.TRAIN_JITTER_SCALES by crop size


def _resample(src, p, out_h, out_w, f, kernel_order):
    """[T,out_h,out_w,3] in [0,1]: clip_ref.sample's taps; kernel_order: lerps of byte differences and a product with 1/255."""
    T, H, W, _ = src.shape
    y0, y1, ly = clip_ref._axis(out_h, p["oy0"], p["sh"], p["rh"], False, f, None, H - 1 - p["sy0"])
    x0, x1, lx = clip_ref._axis(out_w, p["ox0"], p["sw"], p["rw"], bool(p["flip"]), f, None, W - 1 - p["sx0"])
    y0, y1, x0, x1 = y0 + p["sy0"], y1 + p["sy0"], x0 + p["sx0"], x1 + p["sx0"]
    s = src.astype(f)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    a00, a01, a10, a11 = s[:, y0][:, :, x0], s[:, y0][:, :, x1], s[:, y1][:, :, x0], s[:, y1][:, :, x1]
    if kernel_order:
        top, bot = a00 + lx * (a01 - a00), a10 + lx * (a11 - a10)
        return ((top + ly * (bot - top)) * f(np.float32(1.0) / np.float32(255.0))).astype(f)
    one = f(1)
    top, bot = (one - lx) * a00 + lx * a01, (one - lx) * a10 + lx * a11
    return (((one - ly) * top + ly * bot) / f(255)).astype(f)


def _gray(x, gw):
    return gw[2] * x[..., 2] + gw[1] * x[..., 1] + gw[0] * x[..., 0]


def _kernel_mean(g):
    """The frame means of fp32 g [T,h,w] in the order clip_gray_mean_kernel adds: a thread's RUN pixels in x order, the xor
    butterfly over 64 lanes, the block's waves in order, the blocks in order, one division."""
    T, h, w = g.shape
    runs = -(-w // RUN)
    gp = np.zeros((T, h, runs * RUN), dtype=np.float32)
    gp[:, :, :w] = g
    gp = gp.reshape(T, h * runs, RUN)
    th = np.zeros((T, -(-h * runs // THREADS) * THREADS), dtype=np.float32)
    acc = np.zeros((T, h * runs), dtype=np.float32)
    for j in range(RUN):
        acc = acc + gp[:, :, j]
    th[:, :h * runs] = acc
    lanes = th.reshape(T, -1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, np.arange(64) ^ o]
    waves = lanes[:, :, 0].reshape(T, -1, THREADS // 64)
    blocks = waves[:, :, 0]
    for k in range(1, THREADS // 64):
        blocks = blocks + waves[:, :, k]
    total = blocks[:, 0] if blocks.shape[1] == 1 else None
    if total is None:
        total = np.zeros(T, dtype=np.float32)
        for k in range(blocks.shape[1]):
            total = total + blocks[:, k]
    return total / (np.float32(h) * np.float32(w))


def color_stage(x, color, gray_w, f, mutant=None):
    """x [T,h,w,3] by source channel -> (x after the ops and the shift, the mean grey contrast used per frame [T], zeros
    without contrast)."""
    gw = np.asarray(gray_w, dtype=np.float32).astype(f)
    if mutant == "gray_rgb_position":
        gw = gw[::-1]
    ops = list(zip(color["op"], color["alpha"]))
    if mutant == "listed_order":                                  # the permutation ignored: the draws go to the listed kinds
        ops = list(zip(sorted(color["op"]), color["alpha"]))
    elif mutant == "reordered":                                   # NOT a mutant, see the module docstring
        ops = sorted(ops)
    x0, means = x, np.zeros(x.shape[0], dtype=f)
    for kind, alpha in ops:
        a = f(np.float32(alpha)) if f is np.float32 else f(alpha)
        om = f(1) - a
        if mutant == "weights_swapped":
            a, om = om, a
        if kind == BRIGHTNESS:
            x = x * a
            continue
        if kind == SATURATION:
            other = _gray(x, gw)[..., None]
        else:
            g = _gray(x0 if mutant == "mean_before_ops" else x, gw)
            if mutant == "clip_mean":
                means = np.full(x.shape[0], g.mean(dtype=f), dtype=f)
            else:
                means = _kernel_mean(g) if f is np.float32 else g.mean(axis=(1, 2), dtype=f)
            other = means[:, None, None, None]
        x = (x * a + other * om).astype(f)
    shift = np.asarray(color["shift"], dtype=np.float32 if f is np.float32 else np.float64).astype(f)
    if mutant == "pca_same_index":
        shift = shift[::-1]
    return (x + shift).astype(f), means


def sample(src, p, color, out_h, out_w, mean, std, gray_w, reverse, dtype=np.float64, mutant=None):
    """src uint8 [T,H,W,3], p the descriptor fields, color the record's fields (op, alpha, shift by source channel) ->
    ([3,T,out_h,out_w], frame_mean [T]) in `dtype` arithmetic: np.float64 the reference, np.float32 its twin in the kernels'
    order of operations."""
    f = dtype
    m = np.asarray(mean, dtype=np.float32).astype(f)
    s = np.asarray(std, dtype=np.float32).astype(f)
    x = _resample(src, p, out_h, out_w, f, kernel_order=f is np.float32)
    if mutant == "norm_first":
        x, means = color_stage(((x - m) / s).astype(f), color, gray_w, f)
    else:
        x, means = color_stage(x, color, gray_w, f, mutant)
        x = (x * (f(1) / s) + (-m / s)).astype(f) if f is np.float32 else (x - m) / s
    out = np.moveaxis(x[..., ::-1] if reverse else x, -1, 0)
    return np.ascontiguousarray(out, dtype=f), means


def mean_depth(out_h, out_w, any_order=False):
    """The longest chain of additions behind one frame mean: the kernel's order, or the bound of every order of the
    reference's 3 h w terms."""
    if any_order:
        return 3 * out_h * out_w - 1
    nblk = -(-(-(-out_w // RUN) * out_h) // THREADS)
    return RUN + 6 + THREADS // 64 + nblk


def _carry(p, color, out_h, out_w, coords, any_order):
    """(E, M, Em) after the ops: error and magnitude of x in [0,1] units, and the error of the frame mean (0 without
    contrast); see the module docstring."""
    E = 9 * U + (3 * U * ((p["sh"] + 1) + (p["sw"] + 1)) if coords else 0.0)
    M, Em = 1.0, 0.0
    D = mean_depth(out_h, out_w, any_order)
    for kind, a in zip(color["op"], color["alpha"]):
        a = float(a)
        if kind == BRIGHTNESS:
            E, M = abs(a) * E + 2 * U * abs(a) * M, abs(a) * M
            continue
        G = abs(a) + abs(1 - a)
        extra = 8 * U * M
        if kind == CONTRAST:
            Em = E + (8 + D + 1) * U * M
            extra = (8 + D + 1) * U * M
        E, M = G * E + abs(1 - a) * extra + 6 * U * G * M, G * M
    return E, M, Em


def bound(p, color, out_h, out_w, mean, std, ref=None, bf16=False, coords=True, any_order=False):
    """Admissible |result - fp64 reference| of the output (scalar, or per element with bf16)."""
    E, M, _ = _carry(p, color, out_h, out_w, coords, any_order)
    s = max(abs(float(v)) for v in color["shift"])
    E, M = E + U * s + U * (M + s), M + s
    tol = max((E + 4 * U * (M + abs(float(m)))) / abs(float(sd)) for m, sd in zip(mean, std))
    if bf16:
        tol = tol + 2.0 ** -8 * np.abs(ref)
    return tol


def mean_bound(p, color, out_h, out_w, coords=True):
    """Admissible |frame_mean - fp64 reference| for a record with contrast (kernel order)."""
    return _carry(p, color, out_h, out_w, coords, False)[2]


def ratio(got, ref, tol):
    """max |got - ref| / tol: inside the bound iff <= 1."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / tol))


def fixture():
    return np.load(GOLDEN, allow_pickle=False)


# the case on which each of the first five mutants must leave the bound (tests/make_ava_clip_golden.py asserts it)
MUTANT_CASE = {"clip_mean": "order102", "mean_before_ops": "order012", "gray_rgb_position": "order201",
               "pca_same_index": "pca_only", "listed_order": "order210"}


def case_cfg(tag, mixed=False):
    """The config of a fixture case: crop sizes, jitter scales, mean / std, the reference's PCA tables, cfg.AVA overrides."""
    from focus_amd.slowfast.config.defaults import get_cfg
    _, split, crop, ava = CASES[tag]
    cfg = get_cfg()
    cfg.DATA.MEAN, cfg.DATA.STD = list(MEAN), list(STD)
    cfg.DATA.TRAIN_CROP_SIZE = cfg.DATA.TEST_CROP_SIZE = crop
    cfg.DATA.TRAIN_JITTER_SCALES = list(JITTER[crop])
    cfg.DATA.TRAIN_PCA_EIGVAL, cfg.DATA.TRAIN_PCA_EIGVEC = list(EIGVAL), [list(r) for r in EIGVEC]
    cfg.TRAIN.MIXED_PRECISION = mixed
    for k, v in ava.items():
        setattr(cfg.AVA, k, v)
    return cfg


def case_plan(z, tag):
    """(clip, params, color, boxes, the draw that follows) of a fixture case from the host planner under the case's seed."""
    from focus_amd.slowfast.datasets import device_sampling as ds
    cid, split, _, _ = CASES[tag]
    clip = z["clip_" + cid]
    np.random.seed(int(z[tag + ".seed"]))
    p, color, boxes = ds.ava_plan(case_cfg(tag), clip.shape[1], clip.shape[2], z["boxes_" + cid].copy(), split)
    return clip, p, color, boxes, np.random.uniform()
