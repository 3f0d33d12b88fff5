"""TEST INFRASTRUCTURE: a numpy twin of csrc/randaug.hip (include/focus_amd.h states the arithmetic), held to PIL's own
outputs as recorded from the reference's slowfast/datasets/rand_augment.py in tests/golden/randaug.npz
(tests/make_randaug_golden.py) by tests/test_randaug_ref_cpu.py, and held up to the kernels by tests/test_gpu_randaug.py.

Table ops are integer tables (AutoContrast's in Python doubles, as ImageOps computes it), blends are two separately rounded fp32
operations, clamped and truncated, the affine ops evaluate PIL's inverse map at pixel centres in fp64 and resample with its
bilinear / bicubic filters in fp64, operation by operation in the order of PIL's C code.  `mutant=` switches one rule off, to
show that the bounds of the tests can fail."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug.npz")
FILL = (128, 128, 128)
BILINEAR, BICUBIC = 2, 3                  # PIL's codes
POLICY = "rand-m7-n4-mstd0.5-inc1"        # the string of every shipped config

# op codes of include/focus_amd.h (enum focus_randaug_op)
(COPY, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, ROTATE, SHEAR_X,
 SHEAR_Y, TRANSLATE_X, TRANSLATE_Y) = range(16)
OP_OF_NAME = {"AutoContrast": AUTOCONTRAST, "Equalize": EQUALIZE, "Invert": INVERT, "Rotate": ROTATE, "Posterize": POSTERIZE,
              "PosterizeIncreasing": POSTERIZE, "Solarize": SOLARIZE, "SolarizeIncreasing": SOLARIZE, "SolarizeAdd": SOLARIZE_ADD,
              "Color": COLOR, "ColorIncreasing": COLOR, "Contrast": CONTRAST, "ContrastIncreasing": CONTRAST,
              "Brightness": BRIGHTNESS, "BrightnessIncreasing": BRIGHTNESS, "Sharpness": SHARPNESS,
              "SharpnessIncreasing": SHARPNESS, "ShearX": SHEAR_X, "ShearY": SHEAR_Y, "TranslateXRel": TRANSLATE_X,
              "TranslateYRel": TRANSLATE_Y}
AFFINE = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y)
NEEDS_STATS = (AUTOCONTRAST, EQUALIZE, CONTRAST)

# the cases of the fixture: reference function name -> the arguments it is recorded at (the extremes the level maps of the
# shipped policy can reach, both signs, and an interior value)
CASES = {
    "auto_contrast": [()], "equalize": [()], "invert": [()],
    "posterize": [(0,), (1,), (2,), (4,)], "solarize": [(0,), (77,), (256,)], "solarize_add": [(0,), (38,), (110,)],
    "brightness": [(0.1,), (0.63,), (1.37,), (1.9,)], "color": [(0.1,), (0.63,), (1.37,), (1.9,)],
    "contrast": [(0.1,), (0.63,), (1.37,), (1.9,)], "sharpness": [(0.1,), (0.63,), (1.37,), (1.9,)],
    "rotate": [(0.0,), (21.0,), (-21.0,), (7.3,)], "shear_x": [(0.21,), (-0.21,), (0.05,)], "shear_y": [(0.21,), (-0.21,), (0.05,)],
    "translate_x_rel": [(0.315,), (-0.315,), (0.11,)], "translate_y_rel": [(0.315,), (-0.315,), (0.11,)],
}
OP_OF_FN = {"auto_contrast": AUTOCONTRAST, "equalize": EQUALIZE, "invert": INVERT, "posterize": POSTERIZE, "solarize": SOLARIZE,
            "solarize_add": SOLARIZE_ADD, "brightness": BRIGHTNESS, "color": COLOR, "contrast": CONTRAST, "sharpness": SHARPNESS,
            "rotate": ROTATE, "shear_x": SHEAR_X, "shear_y": SHEAR_Y, "translate_x_rel": TRANSLATE_X,
            "translate_y_rel": TRANSLATE_Y}
FRAMES = ("noise24x32", "ramp37x53", "const64x48", "two64x48", "noise37x53")


def frames():
    """The input frames of the fixture, by name: uint8 [H, W, 3]."""
    rng = np.random.RandomState(20271)
    out = {"noise24x32": rng.randint(0, 256, (24, 32, 3)).astype(np.uint8)}
    y, x = np.mgrid[0:37, 0:53]
    out["ramp37x53"] = np.stack([(x * 255) // 52, (y * 255) // 36, ((x + y) * 200) // 88 + 20], -1).astype(np.uint8)
    out["const64x48"] = np.full((64, 48, 3), (90, 17, 201), dtype=np.uint8)
    two = np.where(rng.rand(64, 48, 1) < 0.3, 40, 200).astype(np.uint8)
    out["two64x48"] = np.repeat(two, 3, -1)
    out["noise37x53"] = rng.randint(30, 220, (37, 53, 3)).astype(np.uint8)
    return out


def fixture():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_key(fn, frame, args, resample=None):
    return "op.%s.%s.%s%s" % (fn, frame, "_".join(repr(a) for a in args), "" if resample is None else ".r%d" % resample)


# ---- stats ---------------------------------------------------------------------------------------------------------------
def luminance(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def stats(img):
    """(histograms int64 [3, 256], sum of L): what the stats launch leaves in a frame's workspace slot."""
    return np.stack([np.bincount(img[..., c].reshape(-1), minlength=256) for c in range(3)]), int(luminance(img).sum())


# ---- tables --------------------------------------------------------------------------------------------------------------
def _clip8f(t):
    """PIL's clamp-then-truncate of an fp32 (or fp64) array."""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def blend(d, v, f, mutant=None):
    """Image.blend(degenerate, image, factor) on integer arrays: fp32 product, fp32 sum, clamp, truncate."""
    f = np.float32(f)
    t = np.float32(d) + (f * (np.asarray(v, np.int32) - np.asarray(d, np.int32)).astype(np.float32)).astype(np.float32)
    if mutant == "round_blend":
        t = np.floor(t + np.float32(0.5))
    return _clip8f(t.astype(np.float32))


def table(op, img, farg=0.0, iarg=0):
    """uint8 [3, 256]: the table of a table op for this frame."""
    v = np.arange(256)
    if op == INVERT:
        t = 255 - v
    elif op == POSTERIZE:
        t = v if iarg >= 8 else v & ~((1 << (8 - iarg)) - 1) & 0xff
    elif op == SOLARIZE:
        t = np.where(v < iarg, v, 255 - v)
    elif op == SOLARIZE_ADD:
        t = np.where(v < 128, np.minimum(255, v + iarg), v)
    elif op == BRIGHTNESS:
        t = blend(np.zeros(256, np.int32), v, farg)
    elif op in (AUTOCONTRAST, EQUALIZE):
        hist, _ = stats(img)
        rows = []
        for c in range(3):
            h = [int(n) for n in hist[c]]
            occupied = [i for i in range(256) if h[i]]
            lut = list(range(256))
            if op == AUTOCONTRAST:
                lo, hi = occupied[0], occupied[-1]
                if hi > lo:
                    scale = 255.0 / (hi - lo)
                    offset = -lo * scale
                    lut = [min(255, max(0, int(i * scale + offset))) for i in range(256)]
            elif len(occupied) > 1:
                step = (sum(h) - h[occupied[-1]]) // 255
                if step:
                    n, lut = step // 2, []
                    for i in range(256):
                        lut.append(min(255, n // step))
                        n += h[i]
            rows.append(lut)
        return np.array(rows, dtype=np.uint8)
    else:
        raise ValueError(op)
    return np.repeat(np.asarray(t, dtype=np.uint8)[None], 3, 0)


# ---- affine --------------------------------------------------------------------------------------------------------------
def coefficients(op, arg, w, h):
    """The six coefficients of PIL's inverse map for an affine op on a w x h frame (Image.rotate's own construction for
    ROTATE), or None when PIL returns a plain copy (a rotation by a multiple of 360 degrees)."""
    if op == SHEAR_X:
        return (1.0, float(arg), 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return (1.0, 0.0, 0.0, float(arg), 1.0, 0.0)
    if op == TRANSLATE_X:
        return (1.0, 0.0, float(arg * w), 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return (1.0, 0.0, 0.0, 0.0, 1.0, float(arg * h))
    assert op == ROTATE
    angle = arg % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2.0, h / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def _bicubic1(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, coef, resample, fill=FILL, mutant=None):
    """PIL's Image.transform(size, AFFINE, coef, resample, fillcolor=fill) for resample BILINEAR / BICUBIC, in fp64."""
    H, W = img.shape[:2]
    a = [np.float64(c) for c in coef]
    half = 0.0 if mutant == "corner_sampling" else 0.5
    ys, xs = np.mgrid[0:H, 0:W]
    xc, yc = xs + np.float64(half), ys + np.float64(half)
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    if mutant == "fill_off_by_one":
        outside = (xin < 0) | (xin >= W - 1) | (yin < 0) | (yin >= H - 1)       # the bound of a corner-sampled grid
    else:
        outside = (xin < 0) | (xin >= W) | (yin < 0) | (yin >= H)
    xin, yin = xin - half, yin - half
    x = np.floor(xin).astype(np.int64)
    y = np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    src = img.astype(np.float64)
    cx = lambda v: np.clip(v, 0, W - 1)
    cy = lambda v: np.clip(v, 0, H - 1)
    if resample == BILINEAR:
        lerp = lambda p, q, d: p + (q - p) * d
        x0, x1 = cx(x), cx(x + 1)
        v1 = lerp(src[cy(y), x0], src[cy(y), x1], dx)
        has1 = ((y + 1 >= 0) & (y + 1 < H))[..., None]
        v2 = np.where(has1, lerp(src[cy(y + 1), x0], src[cy(y + 1), x1], dx), v1)
        out = np.trunc(np.clip(lerp(v1, v2, dy), 0, 255)).astype(np.uint8)
    elif resample == BICUBIC:
        x, y = x - 1, y - 1
        xi = [cx(x + k) for k in range(4)]
        rows = []
        for k in range(4):
            yk = cy(y + k)
            v = _bicubic1(src[yk, xi[0]], src[yk, xi[1]], src[yk, xi[2]], src[yk, xi[3]], dx)
            if k:
                v = np.where(((y + k >= 0) & (y + k < H))[..., None], v, rows[k - 1])
            rows.append(v)
        out = _clip8f(_bicubic1(rows[0], rows[1], rows[2], rows[3], dy))
    else:
        raise ValueError("resample %r" % (resample,))
    return np.where(outside[..., None], np.array(fill, dtype=np.uint8), out)


# ---- one op --------------------------------------------------------------------------------------------------------------
def smooth(img):
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 in fp32, accumulated from 0.5 row by row (y+1, y, y-1); the border
    pixels are copied."""
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    f = img.astype(np.float32)
    out = img.copy()
    if img.shape[0] < 3 or img.shape[1] < 3:
        return out
    ss = np.full(f[1:-1, 1:-1].shape, np.float32(0.5), dtype=np.float32)
    for rows, kc in ((f[2:], k1), (f[1:-1], k5), (f[:-2], k1)):
        ss = ss + ((rows[:, :-2] * k1 + rows[:, 1:-1] * kc) + rows[:, 2:] * k1)
    out[1:-1, 1:-1] = _clip8f(ss)
    return out


def apply_op(img, op, farg=0.0, iarg=0, resample=BILINEAR, coef=None, fill=FILL, mutant=None):
    """One op on one uint8 [H, W, 3] frame -> a new frame.  coef None: computed from farg for the affine ops."""
    H, W = img.shape[:2]
    if isinstance(resample, (tuple, list)):                    # a plan's record for one image
        (resample,) = resample
    if op == COPY:
        return img.copy()
    if op in (AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, BRIGHTNESS):
        t = table(op, img, farg, iarg)
        return np.stack([t[c][img[..., c]] for c in range(3)], -1)
    if op == COLOR:
        return blend(luminance(img)[..., None], img, farg, mutant)
    if op == CONTRAST:
        grey = int(stats(img)[1] / (H * W) + 0.5)
        return blend(np.int32(grey), img, farg, mutant)
    if op == SHARPNESS:
        return blend(smooth(img), img, farg, mutant)
    if op in AFFINE:
        if coef is None:
            coef = coefficients(op, farg, W, H)
        if coef is None:
            return img.copy()
        return affine(img, coef, resample, fill, mutant)
    raise ValueError("op %r" % (op,))


def apply_fn(img, fn, args, resample=BILINEAR, mutant=None):
    """The twin of the reference function `fn` of rand_augment.py at `args`."""
    op = OP_OF_FN[fn]
    farg = float(args[0]) if args and op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS) + AFFINE else 0.0
    iarg = int(args[0]) if args and op in (POSTERIZE, SOLARIZE, SOLARIZE_ADD) else 0
    return apply_op(img, op, farg, iarg, resample, mutant=mutant)


def apply_plan(img, layers):
    """A frame through the layer records of a plan ({"op", "farg", "iarg", "resample", "coef"}; None = the gate stayed closed)."""
    for rec in layers:
        if rec is not None:
            img = apply_op(img, rec["op"], rec.get("farg", 0.0), rec.get("iarg", 0), rec.get("resample", BILINEAR), rec.get("coef"))
    return img
