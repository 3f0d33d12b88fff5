"""Loss lookup (mirror of slowfast/models/losses.py:15-121): label-smoothing / plain cross entropy on the fused
focus_xent_ls kernel, soft-target cross entropy (mixup / cutmix targets) on focus_xent_soft, and the EPIC-Kitchens
verb+noun wrapper (EKLoss, losses.py:62-95), and the two binary cross entropies of the multi-label route ("bce",
"bce_logit": losses.py:91-92) on focus_bce_rows."""
from functools import partial

import torch.nn as nn

from focus_amd import ops


class SoftTargetCrossEntropy(nn.Module):
    """losses.py:15-36: sum(-y * log_softmax(x)) per row against a dense [B,V] target; reduction "mean" or "none"."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, x, y):
        if self.reduction not in ("mean", "none"):
            raise NotImplementedError
        return ops.soft_target_ce(x, y, self.reduction)


class LabelSmoothingCrossEntropy(nn.Module):
    def __init__(self, reduction="mean", smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        if reduction != "mean":
            raise NotImplementedError("the reference's LabelSmoothingCrossEntropy always returns the mean "
                                      "(losses.py:53-59); reduction=%r is not used by the train loops" % reduction)
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x, target):
        return ops.label_smoothing_ce(x, target, self.smoothing)


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss (losses.py:92, "bce_logit") against multi-hot or soft targets [B,C]; reduction "mean" or "sum"."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise NotImplementedError("BCEWithLogitsLoss reduction=%r is not used by the train loops ('mean' or 'sum')" % reduction)
        self.reduction = reduction

    def forward(self, x, y):
        return ops.bce_with_logits(x, y, self.reduction)


class BCELoss(nn.Module):
    """nn.BCELoss (losses.py:91, "bce") on probabilities, e.g. a head with MODEL.HEAD_ACT sigmoid; reduction "mean" or "sum"."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise NotImplementedError("BCELoss reduction=%r is not used by the train loops ('mean' or 'sum')" % reduction)
        self.reduction = reduction

    def forward(self, p, y):
        return ops.bce(p, y, self.reduction)


class EKLoss(nn.Module):
    """losses.py:62-95: {'verb_loss', 'noun_loss'} from the two heads' logits and a {'verb','noun'} label dict."""

    def __init__(self, reduction="mean", ce_type="", smoothing=0.1):
        super().__init__()
        self.reduction = reduction
        if ce_type == "soft":
            self.ce_loss = SoftTargetCrossEntropy(reduction=reduction)
        elif ce_type == "label_smoothing":
            self.ce_loss = LabelSmoothingCrossEntropy(reduction=reduction, smoothing=smoothing)
        else:
            self.ce_loss = LabelSmoothingCrossEntropy(reduction=reduction, smoothing=0.0)   # nn.CrossEntropyLoss

    def forward(self, extra_preds, y):
        return {"verb_loss": self.ce_loss(extra_preds["verb"], y["verb"]),
                "noun_loss": self.ce_loss(extra_preds["noun"], y["noun"])}


_LOSSES = {"cross_entropy": partial(LabelSmoothingCrossEntropy, smoothing=0.0),
           "soft_cross_entropy": SoftTargetCrossEntropy,
           "label_smoothing_cross_entropy": LabelSmoothingCrossEntropy,
           "bce": BCELoss,
           "bce_logit": BCEWithLogitsLoss}


def get_loss_func(cfg, state="train"):
    name = cfg.MODEL.LOSS_FUNC
    if state == "val" and name == "soft_cross_entropy":
        name = "cross_entropy"
    if cfg.TRAIN.DATASET == "epickitchens":                       # losses.py:106-114
        if name == "cross_entropy":
            return partial(EKLoss, ce_type="")
        if name == "soft_cross_entropy":
            return partial(EKLoss, ce_type="soft")
        if name == "label_smoothing_cross_entropy":
            return partial(EKLoss, ce_type="label_smoothing", smoothing=cfg.MIXUP.LABEL_SMOOTH_VALUE)
        raise NotImplementedError("%s for epickitchens" % name)
    if name not in _LOSSES:
        raise NotImplementedError("Loss {} is not supported".format(name))
    ret = _LOSSES[name]
    if name == "label_smoothing_cross_entropy":
        ret = partial(ret, smoothing=cfg.MIXUP.LABEL_SMOOTH_VALUE)
    return ret
