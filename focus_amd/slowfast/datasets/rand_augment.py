"""RandAugment for device clips: the host half (mirror of slowfast/datasets/rand_augment.py and of the boxes variant,
boxes_autoaugment/autoaugment.py, of the reference).

The reference's transform takes PIL images on a loader worker.  This one takes none: `RandAugment.plan(size, boxes)` consumes
exactly the reference's random draws, in its order -- `np.random.choice` over the ops, then per op `random.random()` for the
0.5 gate, `random.gauss` when magnitude_std > 0, the level map's own `random.random()` for the sign and, for an affine op
whose resample is the (BILINEAR, BICUBIC) tuple, one `random.choice` per image where `_check_args_tf` makes it -- and
returns what `ops.randaug_apply` runs on the device (csrc/randaug.hip): per layer a record with the op code, its argument,
the resample and the six coefficients of PIL's inverse map.  Boxes (numpy xyxy pixels) move on the host, as
`AugmentOp.__call__` of the boxes variant moves them."""
import math
import random
import re

import numpy as np

_FILL = (128, 128, 128)
_MAX_LEVEL = 10.0
_HPARAMS_DEFAULT = {"translate_const": 250, "img_mean": _FILL}
BILINEAR, BICUBIC = 2, 3                                    # PIL's Image.BILINEAR / Image.BICUBIC
_RANDOM_INTERPOLATION = (BILINEAR, BICUBIC)

# op codes of include/focus_amd.h (enum focus_randaug_op)
(OP_COPY, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_BRIGHTNESS, OP_COLOR,
 OP_CONTRAST, OP_SHARPNESS, OP_ROTATE, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y) = range(16)
AFFINE_OPS = (OP_ROTATE, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y)


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def _rotate_level_to_arg(level, _hparams):
    return (_randomly_negate((level / _MAX_LEVEL) * 30.0),)


def _enhance_level_to_arg(level, _hparams):
    return ((level / _MAX_LEVEL) * 1.8 + 0.1,)


def _enhance_increasing_level_to_arg(level, _hparams):
    level = (level / _MAX_LEVEL) * 0.9
    return (1.0 + _randomly_negate(level),)


def _shear_level_to_arg(level, _hparams):
    return (_randomly_negate((level / _MAX_LEVEL) * 0.3),)


def _translate_rel_level_to_arg(level, hparams):
    translate_pct = hparams.get("translate_pct", 0.45)
    return (_randomly_negate((level / _MAX_LEVEL) * translate_pct),)


def _posterize_level_to_arg(level, _hparams):
    return (int((level / _MAX_LEVEL) * 4),)


def _posterize_increasing_level_to_arg(level, hparams):
    return (4 - _posterize_level_to_arg(level, hparams)[0],)


def _solarize_level_to_arg(level, _hparams):
    return (int((level / _MAX_LEVEL) * 256),)


def _solarize_increasing_level_to_arg(level, _hparams):
    return (256 - _solarize_level_to_arg(level, _hparams)[0],)


def _solarize_add_level_to_arg(level, _hparams):
    return (int((level / _MAX_LEVEL) * 110),)


LEVEL_TO_ARG = {
    "AutoContrast": None, "Equalize": None, "Invert": None, "Rotate": _rotate_level_to_arg,
    "Posterize": _posterize_level_to_arg, "PosterizeIncreasing": _posterize_increasing_level_to_arg,
    "Solarize": _solarize_level_to_arg, "SolarizeIncreasing": _solarize_increasing_level_to_arg,
    "SolarizeAdd": _solarize_add_level_to_arg,
    "Color": _enhance_level_to_arg, "ColorIncreasing": _enhance_increasing_level_to_arg,
    "Contrast": _enhance_level_to_arg, "ContrastIncreasing": _enhance_increasing_level_to_arg,
    "Brightness": _enhance_level_to_arg, "BrightnessIncreasing": _enhance_increasing_level_to_arg,
    "Sharpness": _enhance_level_to_arg, "SharpnessIncreasing": _enhance_increasing_level_to_arg,
    "ShearX": _shear_level_to_arg, "ShearY": _shear_level_to_arg,
    "TranslateXRel": _translate_rel_level_to_arg, "TranslateYRel": _translate_rel_level_to_arg,
}

NAME_TO_OP = {
    "AutoContrast": OP_AUTOCONTRAST, "Equalize": OP_EQUALIZE, "Invert": OP_INVERT, "Rotate": OP_ROTATE,
    "Posterize": OP_POSTERIZE, "PosterizeIncreasing": OP_POSTERIZE, "Solarize": OP_SOLARIZE, "SolarizeIncreasing": OP_SOLARIZE,
    "SolarizeAdd": OP_SOLARIZE_ADD, "Color": OP_COLOR, "ColorIncreasing": OP_COLOR, "Contrast": OP_CONTRAST,
    "ContrastIncreasing": OP_CONTRAST, "Brightness": OP_BRIGHTNESS, "BrightnessIncreasing": OP_BRIGHTNESS,
    "Sharpness": OP_SHARPNESS, "SharpnessIncreasing": OP_SHARPNESS, "ShearX": OP_SHEAR_X, "ShearY": OP_SHEAR_Y,
    "TranslateXRel": OP_TRANSLATE_X, "TranslateYRel": OP_TRANSLATE_Y,
}


# ---- geometry: PIL's inverse map, and the boxes under it -------------------------------------------------------------------
def affine_coefficients(op, arg, size):
    """The six coefficients Image.transform(size, AFFINE, ...) gets from the reference's function for this op on a frame of
    PIL size (w, h); Rotate's are Image.rotate's own construction.  None: PIL returns a plain copy (rotation by 0)."""
    w, h = size
    if op == OP_SHEAR_X:
        return (1.0, float(arg), 0.0, 0.0, 1.0, 0.0)
    if op == OP_SHEAR_Y:
        return (1.0, 0.0, 0.0, float(arg), 1.0, 0.0)
    if op == OP_TRANSLATE_X:
        return (1.0, 0.0, float(arg * w), 0.0, 1.0, 0.0)
    if op == OP_TRANSLATE_Y:
        return (1.0, 0.0, 0.0, 0.0, 1.0, float(arg * h))
    if op != OP_ROTATE:
        raise ValueError("op %r is not affine" % (op,))
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


def _corners(boxes):
    """bbox_util.get_corners: [N,4] xyxy -> [N,8] x1 y1 x2 y1 x1 y2 x2 y2."""
    x1, y1, x2, y2 = (boxes[:, i:i + 1] for i in range(4))
    return np.hstack((x1, y1, x1 + (x2 - x1), y1, x1, y1 + (y2 - y1), x2, y2))


def _enclosing(corners):
    xs, ys = corners[:, 0::2], corners[:, 1::2]
    return np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), 1)


def clip_box(bbox, clip, alpha):
    """bbox_util.clip_box: clip to `clip` (x1 y1 x2 y2); a box that keeps less than `alpha` of its area becomes zeros."""
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    before = area(bbox)
    out = np.stack((np.maximum(bbox[:, 0], clip[0]), np.maximum(bbox[:, 1], clip[1]), np.minimum(bbox[:, 2], clip[2]),
                    np.minimum(bbox[:, 3], clip[3])), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = (before - area(out)) / before
    out[~(delta < (1 - alpha))] = 0
    return out


def rotate_boxes(boxes, angle, size_before):
    """bbox_util.rotate_boxes restated without cv2: getRotationMatrix2D((cx, cy), angle, 1) is [[a, b, (1-a) cx - b cy],
    [-b, a, b cx + (1-a) cy]] with a = cos, b = sin of the angle in degrees; the rotated canvas is (nW, nH) as rotate_im sizes
    it, the corners go through the matrix shifted to that canvas's centre, the enclosing boxes are centre-cropped back to
    (w, h) and clipped with the 25 % rule."""
    boxes = np.asarray(boxes, dtype=np.float64)
    w, h = size_before
    cx, cy = w // 2, h // 2
    a, b = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)
    cos, sin = abs(M[0, 0]), abs(M[0, 1])
    nW, nH = int(h * sin + w * cos), int(h * cos + w * sin)
    M[0, 2] += nW / 2 - cx
    M[1, 2] += nH / 2 - cy
    pts = _corners(boxes).reshape(-1, 2)
    pts = np.hstack((pts, np.ones((pts.shape[0], 1))))
    new = _enclosing(np.dot(M, pts.T).T.reshape(-1, 8))
    w_delta, h_delta = (nW - w) / 2, (nH - h) / 2
    new[:, [0, 2]] = np.clip(new[:, [0, 2]], w_delta, nW - w_delta) - w_delta
    new[:, [1, 3]] = np.clip(new[:, [1, 3]], h_delta, nH - h_delta) - h_delta
    return clip_box(new, [0, 0, w, h], 0.25)


def shear_boxes(boxes, op, factor, size_before):
    """Boxes under the pixel transform the frame gets here (Deviations: the reference goes through imgaug).
    PIL's matrix maps an output point to its source, (x, y) -> (x + f y, y) for ShearX and (x, f x + y) for ShearY; a box's
    corners go through the inverse, and the enclosing box is clipped to the frame."""
    boxes = np.asarray(boxes, dtype=np.float64)
    w, h = size_before
    c = _corners(boxes)
    if op == OP_SHEAR_X:
        c[:, 0::2] = c[:, 0::2] - factor * c[:, 1::2]
    else:
        c[:, 1::2] = c[:, 1::2] - factor * c[:, 0::2]
    out = _enclosing(c)
    out[:, [0, 2]] = np.clip(out[:, [0, 2]], 0, w)
    out[:, [1, 3]] = np.clip(out[:, [1, 3]], 0, h)
    return out


def move_boxes(boxes, op, arg, size_before):
    """One frame's [O,4] boxes under one op (boxes_autoaugment.NAME_TO_OP): identity for the colour ops."""
    w, h = size_before
    if op == OP_ROTATE:
        return rotate_boxes(boxes, arg, size_before)
    if op in (OP_SHEAR_X, OP_SHEAR_Y):
        return boxes if arg == 0 else shear_boxes(boxes, op, arg, size_before)
    if op == OP_TRANSLATE_X:
        out = boxes.copy()
        out[:, [0, 2]] = boxes[:, [0, 2]] - w * arg
        return out
    if op == OP_TRANSLATE_Y:
        out = boxes.copy()
        out[:, [1, 3]] = boxes[:, [1, 3]] - h * arg
        return out
    return boxes


# ---- the policy ------------------------------------------------------------------------------------------------------------
class AugmentOp:
    """One op of the policy.  plan() is AugmentOp.__call__ of the reference without the images."""

    def __init__(self, name, prob=0.5, magnitude=10, hparams=None, seed=None):
        hparams = hparams or _HPARAMS_DEFAULT
        self.name = name
        self.op = NAME_TO_OP[name]
        self.level_fn = LEVEL_TO_ARG[name]
        self.prob = prob
        self.magnitude = magnitude
        self.hparams = hparams.copy()
        self.fill = tuple(hparams["img_mean"]) if "img_mean" in hparams else _FILL
        self.resample = hparams["interpolation"] if "interpolation" in hparams else _RANDOM_INTERPOLATION
        self.magnitude_std = self.hparams.get("magnitude_std", 0)
        self.seed = seed

    def plan(self, size, boxes=None, n_images=1):
        """-> (record or None, boxes).  None: the gate stayed closed.  The record holds name, op, farg, iarg, fill and, per
        image, resample (a tuple of n_images codes) and coef (the six coefficients, or None for a plain copy)."""
        if self.seed is not None:
            np.random.seed(self.seed)
            random.seed(self.seed)
        if self.prob < 1.0 and random.random() > self.prob:
            return None, boxes
        magnitude = self.magnitude
        if self.magnitude_std and self.magnitude_std > 0:
            magnitude = random.gauss(magnitude, self.magnitude_std)
        magnitude = min(_MAX_LEVEL, max(0, magnitude))
        args = self.level_fn(magnitude, self.hparams) if self.level_fn is not None else ()
        rec = {"name": self.name, "op": self.op, "farg": 0.0, "iarg": 0, "fill": self.fill, "resample": (BILINEAR,) * n_images,
               "coef": None}
        if args:
            if isinstance(args[0], int):
                rec["iarg"] = args[0]
            else:
                rec["farg"] = float(args[0])
        if self.op in AFFINE_OPS:
            if isinstance(self.resample, (list, tuple)):                  # _check_args_tf: one draw per image
                rec["resample"] = tuple(random.choice(self.resample) for _ in range(n_images))
            else:
                rec["resample"] = (self.resample,) * n_images
            rec["coef"] = affine_coefficients(self.op, rec["farg"], size)
        if boxes is not None:
            boxes = np.asarray(boxes)
            zero = np.repeat((boxes == 0).all(axis=-1, keepdims=True), 4, -1)
            arg = rec["farg"] if self.op in AFFINE_OPS else 0.0
            moved = np.stack([move_boxes(boxes[i], self.op, arg, size) for i in range(len(boxes))])
            moved[zero] = 0
            boxes = moved
        return rec, boxes


_RAND_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
                    "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]

_RAND_INCREASING_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing",
                               "SolarizeAdd", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing",
                               "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]

_RAND_CHOICE_WEIGHTS_0 = {"Rotate": 0.3, "ShearX": 0.2, "ShearY": 0.2, "TranslateXRel": 0.1, "TranslateYRel": 0.1, "Color": 0.025,
                          "Sharpness": 0.025, "AutoContrast": 0.025, "Solarize": 0.005, "SolarizeAdd": 0.005, "Contrast": 0.005,
                          "Brightness": 0.005, "Equalize": 0.005, "Posterize": 0, "Invert": 0}


def _select_rand_weights(weight_idx=0, transforms=None):
    transforms = transforms or _RAND_TRANSFORMS
    assert weight_idx == 0
    probs = [_RAND_CHOICE_WEIGHTS_0[k] for k in transforms]
    probs /= np.sum(probs)
    return probs


def rand_augment_ops(magnitude=10, hparams=None, transforms=None, seed=None):
    hparams = hparams or _HPARAMS_DEFAULT
    transforms = transforms or _RAND_TRANSFORMS
    return [AugmentOp(name, prob=0.5, magnitude=magnitude, hparams=hparams, seed=seed) for name in transforms]


class RandAugment:
    def __init__(self, ops, num_layers=2, choice_weights=None):
        self.ops = ops
        self.num_layers = num_layers
        self.choice_weights = choice_weights

    def __call__(self, img, boxes=None):
        raise TypeError("this RandAugment plans for the device: call plan(size, boxes) and run the result with "
                        "focus_amd.ops.randaug_apply (datasets/device_sampling.augment_clips does both)")

    def plan(self, size, boxes=None, n_images=1):
        """size: PIL's (w, h).  boxes: None, [O,4] (one image) or [n_images,O,4].  -> (layers, boxes): num_layers records
        (None where the gate stayed closed), and the boxes as the reference would return them, in the shape given."""
        ops = np.random.choice(self.ops, self.num_layers, replace=self.choice_weights is None, p=self.choice_weights)
        flat = boxes is not None and np.asarray(boxes).ndim == 2
        if boxes is not None:
            boxes = np.asarray(boxes)[None] if flat else np.asarray(boxes)
        layers = []
        for op in ops:
            rec, boxes = op.plan(size, boxes, n_images)
            layers.append(rec)
        if flat:
            boxes = boxes[0]
        return layers, boxes


def rand_augment_transform(config_str, hparams, seed=None):
    """The reference's string grammar: sections separated by '-', the first is 'rand'; m (magnitude), n (layers), w (weight
    set), mstd (magnitude noise), inc (the increasing list; as in the reference ANY value switches it on)."""
    magnitude = _MAX_LEVEL
    num_layers = 2
    weight_idx = None
    transforms = _RAND_TRANSFORMS
    config = config_str.split("-")
    if config[0] != "rand":
        raise ValueError("RandAugment config %r does not start with 'rand'" % (config_str,))
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            hparams.setdefault("magnitude_std", float(val))
        elif key == "inc":
            if bool(val):
                transforms = _RAND_INCREASING_TRANSFORMS
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "w":
            weight_idx = int(val)
    if num_layers < 1:
        raise ValueError("RandAugment config %r asks for %d layers" % (config_str, num_layers))
    if weight_idx not in (None, 0):
        raise ValueError("RandAugment config %r: only weight set 0 exists" % (config_str,))
    ra_ops = rand_augment_ops(magnitude=magnitude, hparams=hparams, transforms=transforms, seed=seed)
    choice_weights = None if weight_idx is None else _select_rand_weights(weight_idx)
    return RandAugment(ra_ops, num_layers, choice_weights=choice_weights)
