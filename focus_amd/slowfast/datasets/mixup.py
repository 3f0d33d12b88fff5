"""Mixup / CutMix of a batch of clips (mirror of slowfast/datasets/mixup.py:22-192, itself after timm's data/mixup.py).

The surface, the semantics and the order of the draws from numpy's global generator are the reference's, so one
np.random.seed gives one lam, mode and box on both sides.  On the device the pixels and the targets go through
csrc/mixup.hip (ops.mixup_blend_, ops.cutmix_paste_, ops.mixup_target): one in-place pass over the clips, pair (i, B-1-i)
at a time, instead of flip / mul_ / mul_ / add_ over the whole batch, and one launch for the dense target, with ATen's bits.
CPU tensors (data workers, tests) take the plain torch expressions."""
import numpy as np
import torch

from focus_amd import ops


def convert_to_one_hot(targets, num_classes, on_value=1.0, off_value=0.0):
    """[N] class indices -> fp32 [N, num_classes] filled with off_value, on_value at the class (mixup.py:22-37)."""
    idx = targets.long().view(-1, 1)
    dense = torch.full((idx.shape[0], num_classes), off_value, device=idx.device)
    return dense.scatter_(1, idx, on_value)


def mixup_target(target, num_classes, lam=1.0, smoothing=0.0):
    """Smoothed one-hot rows of `target` and of `target.flip(0)`, mixed lam : 1 - lam (mixup.py:40-64)."""
    if target.is_cuda:
        return ops.mixup_target(target, num_classes, lam, smoothing)
    off_value = smoothing / num_classes
    on_value = 1.0 - smoothing + off_value
    t1 = convert_to_one_hot(target, num_classes, on_value, off_value)
    t2 = convert_to_one_hot(target.flip(0), num_classes, on_value, off_value)
    return t1 * lam + t2 * (1.0 - lam)


def rand_bbox(img_shape, lam, margin=0.0, count=None):
    """A box holding the share 1 - lam of the frame around a random centre, clipped to the frame: (yl, yh, xl, xh)
    (mixup.py:67-87).  Draws the centre's y, then its x."""
    h, w = img_shape[-2:]
    side = np.sqrt(1 - lam)
    box_h, box_w = int(h * side), int(w * side)
    my, mx = int(margin * box_h), int(margin * box_w)
    cy = np.random.randint(my, h - my, size=count)
    cx = np.random.randint(mx, w - mx, size=count)
    yl, yh = (np.clip(cy + d, 0, h) for d in (-(box_h // 2), box_h // 2))
    xl, xh = (np.clip(cx + d, 0, w) for d in (-(box_w // 2), box_w // 2))
    return yl, yh, xl, xh


def get_cutmix_bbox(img_shape, lam, correct_lam=True, count=None):
    """((yl, yh, xl, xh), lam); with correct_lam, lam becomes the share of the frame the clipped box leaves
    (mixup.py:90-106)."""
    yl, yh, xl, xh = rand_bbox(img_shape, lam, count=count)
    if correct_lam:
        lam = 1.0 - (yh - yl) * (xh - xl) / float(img_shape[-2] * img_shape[-1])
    return (yl, yh, xl, xh), lam


class MixUp:
    """Batch-level mixup and / or cutmix for videos (mixup.py:109-192).  `mixup_fn(x, target)` mixes x IN PLACE with its
    batch-reversed self and returns (x, dense target); `target` is a [B] label tensor, or a dict of them with `num_classes`
    a dict of the same keys (EPIC-Kitchens)."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, mix_prob=1.0, switch_prob=0.5, correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.mix_prob = mix_prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.correct_lam = correct_lam

    def _get_mixup_params(self):
        """(lam, use_cutmix).  Draws: rand(); rand() again only when both alphas are positive; beta(alpha, alpha)."""
        lam, use_cutmix = 1.0, False
        if np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = np.random.rand() < self.switch_prob
                alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            elif self.mixup_alpha > 0.0:
                alpha = self.mixup_alpha
            elif self.cutmix_alpha > 0.0:
                use_cutmix, alpha = True, self.cutmix_alpha
            lam = float(np.random.beta(alpha, alpha))
        return lam, use_cutmix

    def _mix_batch(self, x):
        lam, use_cutmix = self._get_mixup_params()
        if lam == 1.0:                                   # nothing to mix: no launch on the clips
            return 1.0
        if use_cutmix:
            (yl, yh, xl, xh), lam = get_cutmix_bbox(x.shape, lam, correct_lam=self.correct_lam)
            if x.is_cuda:
                ops.cutmix_paste_(x, yl, yh, xl, xh)
            else:
                x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
        elif x.is_cuda:
            ops.mixup_blend_(x, lam)
        else:
            x_flipped = x.flip(0).mul_(1.0 - lam)
            x.mul_(lam).add_(x_flipped)
        return lam

    def __call__(self, x, target):
        assert len(x) > 1, "Batch size should be greater than 1 for mixup."
        lam = self._mix_batch(x)
        if isinstance(target, dict):
            target = {k: mixup_target(v, self.num_classes[k], lam, self.label_smoothing) for k, v in target.items()}
        else:
            target = mixup_target(target, self.num_classes, lam, self.label_smoothing)
        return x, target
