"""Random erasing of a normalised clip (mirror of slowfast/datasets/random_erasing.py:18-180, itself after timm's
data/random_erasing.py).

The surface, the semantics and the order of the draws from Python's `random` are the reference's, so one random.seed gives
the same rectangles on both sides.  The planning is split from the writing: `plan` makes every draw and returns the
rectangles, and on the device ONE launch of csrc/random_erase.hip writes them (ops.random_erase_).  There the fill comes from
the build-owned counter-based generator: the distribution is the reference's N(0,1), the draws are not (the reference
itself draws them from torch's CPU generator).  CPU tensors (data workers, tests) take the reference's torch expressions,
and with torch.manual_seed its bits."""
import math
import random

import torch

from focus_amd import ops


def _get_pixels(per_pixel, rand_color, patch_size, dtype=torch.float32, device="cuda"):
    """The fill of one frame's rectangle (random_erasing.py:18-31)."""
    if per_pixel:
        return torch.empty(patch_size, dtype=dtype, device=device).normal_()
    if rand_color:
        return torch.empty((patch_size[0], 1, 1), dtype=dtype, device=device).normal_()
    return torch.zeros((patch_size[0], 1, 1), dtype=dtype, device=device)


class RandomErasing:
    """Erases rectangles of an image or of the frames of a clip that has been normalised (random_erasing.py:34-180).
    mode 'const' fills with 0, 'rand' with one normal value per channel (and frame), 'pixel' with one per element;
    max_count rectangles per call share the area; with num_splits > 1 the first n // num_splits frames stay clean; cube
    erases one rectangle through all frames, otherwise every frame draws its own.  `device` is accepted for the
    reference's signature: the fill is made where the input lives."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="const",
                 min_count=1, max_count=None, num_splits=0, device="cuda", cube=True):
        self.probability = probability
        self.min_area = min_area
        self.max_area = max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count = min_count
        self.max_count = max_count or min_count
        self.num_splits = num_splits
        mode = mode.lower()
        self.rand_color = False
        self.per_pixel = False
        self.cube = cube
        if mode == "rand":
            self.rand_color = True
        elif mode == "pixel":
            self.per_pixel = True
        else:
            assert not mode or mode == "const"
        self.device = device

    @property
    def mode(self):
        return "pixel" if self.per_pixel else "rand" if self.rand_color else "const"

    def _plan_one(self, t0, t1, img_h, img_w, attempts):
        """The draws of one `_erase` (attempts 10) or `_erase_cube` (attempts 100) call, in its order: the gate, the count when
        min_count != max_count, per rectangle up to `attempts` pairs of uniforms and, on a fit, two randints."""
        if random.random() > self.probability:
            return []
        area = img_h * img_w
        count = self.min_count if self.min_count == self.max_count else random.randint(self.min_count, self.max_count)
        out = []
        for _ in range(count):
            for _ in range(attempts):
                target_area = random.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < img_w and h < img_h:
                    top = random.randint(0, img_h - h)
                    left = random.randint(0, img_w - w)
                    out.append(dict(t0=t0, t1=t1, top=top, left=left, h=h, w=w))
                    break
        return out

    def plan(self, n, img_h, img_w):
        """Every draw `__call__` makes from `random` for an [n, C, img_h, img_w] input (n None: a [C, img_h, img_w] image),
        without touching a pixel -> the rectangles in the order the reference writes them: mappings with the frames
        [t0, t1) and top, left, h, w.  A rectangle may be empty (h or w 0 on tiny frames), as in the reference."""
        if n is None:
            return self._plan_one(0, 1, img_h, img_w, 10)
        batch_start = n // self.num_splits if self.num_splits > 1 else 0
        if self.cube:
            return self._plan_one(batch_start, n, img_h, img_w, 100)
        out = []
        for i in range(batch_start, n):
            out += self._plan_one(i, i + 1, img_h, img_w, 10)
        return out

    def _erase_device(self, input, items):
        """One launch for the rectangles of a device tensor: [T,C,H,W] contiguous, the permuted view of a contiguous
        [C,T,H,W] clip that ssv2.py:444 passes, or a contiguous [C,H,W] image."""
        items = [dict(it, clip=0) for it in items if it["h"] > 0 and it["w"] > 0 and it["t0"] < it["t1"]]
        if input.dim() == 3 and input.is_contiguous():
            x, layout = input[None, None], "BTCHW"
        elif input.dim() == 4 and input.is_contiguous():
            x, layout = input[None], "BTCHW"
        elif input.dim() == 4 and input.permute(1, 0, 2, 3).is_contiguous():
            x, layout = input.permute(1, 0, 2, 3)[None], "BCTHW"
        else:
            raise ValueError("RandomErasing on the device takes a contiguous [T,C,H,W] or [C,H,W] tensor or the permuted "
                             "view of a contiguous [C,T,H,W] clip; got strides %s for shape %s" % (
                                 tuple(input.stride()), tuple(input.shape)))
        ops.random_erase_(x, items, self.mode, layout)

    def __call__(self, input):
        if len(input.size()) == 3:
            n, (chan, img_h, img_w) = None, input.size()
        else:
            n, chan, img_h, img_w = input.size()
        items = self.plan(n, img_h, img_w)
        if input.is_cuda:
            if items:
                self._erase_device(input, items)
            return input
        frames = input[None] if n is None else input
        for it in items:                                   # the reference's writes and its torch draws, in its order
            for i in range(it["t0"], it["t1"]):
                frames[i][:, it["top"]:it["top"] + it["h"], it["left"]:it["left"] + it["w"]] = _get_pixels(
                    self.per_pixel, self.rand_color, (chan, it["h"], it["w"]), dtype=input.dtype, device=input.device)
        return input
