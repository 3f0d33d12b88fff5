"""TEST INFRASTRUCTURE: CPU twin of csrc/mixup.hip and the cases of tests/golden/mixup.npz (tests/make_mixup_golden.py).

The twin states the kernels' contract in numpy / torch, independently of the ATen expressions of the reference:
  blend   out[i] = r(r(x[i] lam) + r(x[B-1-i] oml)), lam / oml the fp32 roundings of the doubles lam and 1.0 - lam, r() one
          rounding to the tensor's type (fp32 arithmetic), three separately rounded operations, no fma;
  paste   the rectangle of sample i comes from sample B-1-i, everything else stays;
  target  r(r(t1 lam) + r(t2 oml)) over the smoothed one-hot rows of labels and labels.flip(0), all fp32;
  soft CE sum(-y log_softmax(x)) per row in fp64 and the gradient of its mean over rows, (softmax sum(y) - y) / R;
  collapse the reference's own lines (tools/train_net.py:131-143) for one head, run on the CPU.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixup.npz")

H, W = 8, 10                      # frame of the fixture's clips [B,3,2,H,W]
NUM_CLASSES = 5
EK_CLASSES = {"verb": 97, "noun": 300}

# name -> (B, MixUp keyword arguments, what the seed search looks for)
CASES = {
    "blend_even":      (4, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "blend"),
    "blend_odd":       (3, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "blend"),
    "cutmix_interior": (4, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "interior"),
    "cutmix_clipped":  (3, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "clipped"),
    "cutmix_empty":    (2, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "empty"),
    "no_mix":          (2, dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.0), "none"),
    "mixup_only":      (2, dict(mixup_alpha=0.8, cutmix_alpha=0.0), "blend"),
    "cutmix_only":     (2, dict(mixup_alpha=0.0, cutmix_alpha=1.0, label_smoothing=0.0), "cutmix"),
    "ek_dict":         (4, dict(mixup_alpha=0.8, cutmix_alpha=1.0), "blend"),
}


def fixture():
    return np.load(GOLDEN, allow_pickle=False)


def case_args(name):
    """MixUp keyword arguments of a case, num_classes included."""
    kw = dict(CASES[name][1])
    kw["num_classes"] = dict(EK_CLASSES) if name == "ek_dict" else NUM_CLASSES
    return kw


def f32(v):
    """The fp32 rounding of a host double, as a 0-dim fp32 tensor."""
    return torch.tensor(float(v), dtype=torch.float64).to(torch.float32)


def _r(v, dtype):
    return v.to(dtype).to(torch.float32)


def blend(x, lam):
    """x [B, ...] fp32 or bf16 (CPU) -> the mixed batch, same dtype.  x is not modified."""
    lam = float(lam)
    l, o = f32(lam), f32(1.0 - lam)
    a, b = x.to(torch.float32), x.flip(0).to(torch.float32)
    return _r(_r(a * l, x.dtype) + _r(b * o, x.dtype), x.dtype).to(x.dtype)


def paste(x, yl, yh, xl, xh):
    out = x.clone()
    out[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
    return out


def target(labels, num_classes, lam, smoothing):
    """labels: int64 numpy [B] -> float32 numpy [B, num_classes]."""
    lam = float(lam)
    off = np.float32(smoothing / num_classes)
    on = np.float32(1.0 - smoothing + smoothing / num_classes)
    l, o = np.float32(lam), np.float32(1.0 - lam)
    cols = np.arange(num_classes)[None, :]
    t1 = np.where(cols == np.asarray(labels)[:, None], on, off).astype(np.float32)
    t2 = np.where(cols == np.asarray(labels)[::-1][:, None], on, off).astype(np.float32)
    return (t1 * l).astype(np.float32) + (t2 * o).astype(np.float32)


def soft_ce(logits, y):
    """fp64: (loss rows [R], d(mean of the rows) / d(logits) [R,V]) for logits, y of any float type on the CPU."""
    x = logits.detach().double().cpu()
    y = y.detach().double().cpu()
    logp = torch.log_softmax(x, dim=-1)
    loss = (-y * logp).sum(-1)
    grad = (logp.exp() * y.sum(-1, keepdim=True) - y) / x.shape[0]
    return loss, grad


def collapse(preds, labels):
    """train_net.py:131-143 for one head on CPU copies: (predictions with the runner-up folded into the winner, winner)."""
    preds, labels = preds.detach().cpu().clone(), labels.detach().cpu()
    _vals, inds = torch.topk(labels, 2, dim=1, largest=True, sorted=True)
    rows = torch.arange(labels.shape[0])
    preds[rows, inds[:, 0]] += preds[rows, inds[:, 1]]
    preds[rows, inds[:, 1]] = 0.0
    return preds, inds[:, 0]
