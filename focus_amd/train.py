"""One optimizer step of the supervised loop, in the reference's order (tools/train_net.py:68-121):
H2D -> forward -> loss -> NaN check -> zero_grad -> backward (DDP all-reduce overlapped) -> clip-norm -> step.

Differences that follow from the MI355X design and are deliberate:
  * TRAIN.MIXED_PRECISION selects bf16 storage with fp32 accumulation inside the HIP kernels instead of fp16
    autocast, so no GradScaler is needed (scale/unscale/update are identities);
  * the per-scalar blocking metric all-reduces (train_net.py:247-250) are packed into one collective
    (focus_amd/slowfast/utils/distributed.py:all_reduce).
"""
import os

import torch

from .slowfast.utils import misc


def train_step(model, optimizer, loss_fun, inputs, labels, meta, cfg, check_nan=True, stats=None):
    """`stats`: a meters.StepStats.  The step's loss (for epickitchens also verb_loss and noun_loss), the top-k counts and the
    NaN guard then go into its device tables by one launch right after the loss; the host NaN check is not made whatever
    `check_nan` says, and a NaN surfaces at the next stats.read().  Labels may be the dense rows of mixup.  Under
    cfg.DATA.MULTI_LABEL the labels are multi-hot rows, which have no top-k: the loss and the NaN guard alone are kept
    (train_net.py:234-238), the top-k columns stay zero.  Under cfg.DETECTION.ENABLE the model also takes meta["boxes"]
    ([K,5]: batch index, x1, y1, x2, y2) and returns one row per box; the reference computes no top-k there either (:151)."""
    if cfg.DETECTION.ENABLE:
        preds = model(inputs, meta, bboxes=meta["boxes"])         # train_net.py:83-84
    else:
        preds = model(inputs, meta)                               # train_net.py:86
    extra_preds = None
    if isinstance(preds, tuple):                                  # :87-88 (EK: (verb, {'verb','noun'}))
        preds, extra_preds = preds
    if cfg.TRAIN.DATASET == "epickitchens":                       # :95-97
        loss_dict = loss_fun(extra_preds, labels)
        loss = loss_dict["verb_loss"] + loss_dict["noun_loss"]
    else:
        loss = loss_fun(preds, labels)                            # :99
    if stats is not None:
        if cfg.TRAIN.DATASET == "epickitchens":
            stats.update(extra_preds, labels, loss, (loss_dict["verb_loss"], loss_dict["noun_loss"]))
        elif cfg.DATA.MULTI_LABEL or cfg.DETECTION.ENABLE:
            stats.update(None, None, loss, batch=preds.shape[0])
        else:
            stats.update(preds, labels, loss)
    elif check_nan:
        misc.check_nan_losses(float(loss.detach()))                        # :102 (host sync, as in the reference)
    optimizer.zero_grad(set_to_none=True)                         # :105
    loss.backward()                                               # :106
    from .slowfast.models import optimizer as optim
    fused = optim.fused_route(model, optimizer)                   # FusedAdam / FusedSGD holding every trainable parameter
    if cfg.SOLVER.CLIP_GRAD_VAL and fused:
        optimizer.step_clipped(clip_value=cfg.SOLVER.CLIP_GRAD_VAL)                         # :108-111 + :120 in one pass
        return preds, loss
    elif cfg.SOLVER.CLIP_GRAD_VAL:
        torch.nn.utils.clip_grad_value_(model.parameters(), cfg.SOLVER.CLIP_GRAD_VAL)      # :108-111
    elif cfg.SOLVER.CLIP_GRAD_L2NORM and hasattr(optimizer, "step_clipped") and (
            fused or not isinstance(optimizer, (optim.FusedAdam, optim.FusedSGD))):
        # :112-120 as one multi-tensor pass (optimizer.Fused*: norm, clip, update, bf16 shadows; csrc/optim.hip)
        optimizer.step_clipped(cfg.SOLVER.CLIP_GRAD_L2NORM)
        return preds, loss
    elif cfg.SOLVER.CLIP_GRAD_L2NORM:
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.SOLVER.CLIP_GRAD_L2NORM)    # :112-117
    optimizer.step()                                              # :120
    return preds, loss


def build_mixup(cfg):
    """The MixUp object of train_net.py:58-66, or None when MIXUP.ENABLE is off."""
    if not cfg.MIXUP.ENABLE:
        return None
    from .slowfast.datasets.mixup import MixUp
    return MixUp(mixup_alpha=cfg.MIXUP.ALPHA, cutmix_alpha=cfg.MIXUP.CUTMIX_ALPHA, mix_prob=cfg.MIXUP.PROB,
                 switch_prob=cfg.MIXUP.SWITCH_PROB, label_smoothing=cfg.MIXUP.LABEL_SMOOTH_VALUE,
                 num_classes=misc.get_num_classes(cfg))


def mixup_collapse(preds, labels):
    """train_net.py:123-149: fold mixed dense labels back for the top-k metrics.  Per head, the two largest entries of a
    label row are the mixed pair: the runner-up's score is added into the winner's column of a detached copy of the
    predictions and then zeroed, and the label becomes the winner's index.  Tensors, or the EK dicts of them (`preds` is
    then the {'verb','noun'} logits dict).  [B,V] logging work in plain torch; ties in a label row have no defined order."""
    if isinstance(labels, dict):
        pairs = {k: mixup_collapse(preds[k], labels[k]) for k in labels}
        return {k: p for k, (p, _) in pairs.items()}, {k: l for k, (_, l) in pairs.items()}
    top2 = torch.topk(labels, 2, dim=1, largest=True, sorted=True).indices
    rows = torch.arange(labels.shape[0], device=preds.device)
    first, second = top2[:, 0].to(preds.device), top2[:, 1].to(preds.device)
    preds = preds.detach().clone()
    preds[rows, first] += preds[rows, second]
    preds[rows, second] = 0.0
    return preds, top2[:, 0]


def train_iter(model, optimizer, loss_fun, inputs, labels, meta, cfg, mixup_fn=None, check_nan=True, stats=None):
    """One iteration of train_net.py:78-149 around the unchanged train_step: the optional mixup of inputs[0] and the labels
    (:78-80), the step (:82-121), and with mixup the collapse of the dense labels for the metrics (:123-149).  Returns
    (preds, labels, loss) ready for metrics.topk_errors; for epickitchens `preds` is the {'verb','noun'} dict when mixing
    was on (what the reference scores there), else what train_step returned.
    With `stats` (a meters.StepStats, see train_step) the dense labels go straight into its kernel, which collapses them
    itself: there is no mixup_collapse, and the predictions and labels are returned as the step used them."""
    if mixup_fn is not None:
        inputs[0], labels = mixup_fn(inputs[0], labels)
    if stats is not None:
        preds, loss = train_step(model, optimizer, loss_fun, inputs, labels, meta, cfg, check_nan=check_nan, stats=stats)
        return preds, labels, loss
    if mixup_fn is None or cfg.TRAIN.DATASET != "epickitchens":
        preds, loss = train_step(model, optimizer, loss_fun, inputs, labels, meta, cfg, check_nan=check_nan)
    else:
        # train_step hands back the verb logits alone; the collapse needs both heads, so keep the forward's dict
        kept = {}
        hook = model.register_forward_hook(lambda _m, _i, out: kept.update(out[1]) if isinstance(out, tuple) else None)
        try:
            preds, loss = train_step(model, optimizer, loss_fun, inputs, labels, meta, cfg, check_nan=check_nan)
        finally:
            hook.remove()
        preds = kept
    if mixup_fn is not None:
        preds, labels = mixup_collapse(preds, labels)
    return preds, labels, loss


def slot_train_step(model, optimizer, video, global_step, cfg, noise=None, stats=None, raw_attns=False):
    """One iteration of slot_train_epoch (tools/steve_train_net.py:57-126): schedules -> forward -> mse + cross_entropy ->
    NaN check -> zero_grad -> backward -> clip-norm -> step.  Returns (loss, mse, cross_entropy, recon, attns, tau).
    TRAIN.MIXED_PRECISION selects bf16 storage inside the model (no autocast / GradScaler: see the module docstring).
    `stats`: a meters.StepStats(device, ks=(), aux_names=("mse", "cross_entropy")); loss, mse and cross_entropy then go into
    its device tables and the host NaN check is left to the next stats.read().
    `raw_attns`: the forward runs with attns="raw", so `attns` is the slot update's attention [B,T,N,K] and the fp32 overlays
    [B,T,K,C,H,W], which the loop looks at once per epoch, are not made; everything else is the same bits."""
    import math
    from .slowfast.models import optimizer as optim
    from .slowfast.utils import lr_policy as lrp
    so = cfg.SLOTS_OPTIM
    tau = lrp.cosine_anneal(global_step, so.TAU_START, so.TAU_FINAL, 0, so.TAU_STEPS)                # :60-66
    lr_warmup_factor_enc = lrp.linear_warmup(global_step, 0.0, 1.0, 0.0, so.WARMUP_STEPS)             # :68-73
    lr_warmup_factor_dec = lrp.linear_warmup(global_step, 0.0, 1.0, 0, so.WARMUP_STEPS)               # :75-80
    lr_decay_factor = math.exp(global_step / so.HALF_LIFE * math.log(0.5))                            # :82
    optim.set_slot_lr(optimizer, cfg, lr_decay_factor, lr_warmup_factor_enc, lr_warmup_factor_dec)    # :85-89
    kw = {} if noise is None else {"noise": noise}
    if raw_attns:
        kw["attns"] = "raw"
    recon, cross_entropy, mse, attns = model(video, tau, cfg.SLOTS.HARD, **kw)                        # :98
    mse = mse.mean()                                                                                  # :101-102
    cross_entropy = cross_entropy.mean()
    loss = mse + cross_entropy                                                                        # :104
    if stats is not None:
        stats.update(None, None, loss, (mse, cross_entropy), batch=video.shape[0])
    else:
        misc.check_nan_losses(float(loss.detach()))                                                   # :108
    optimizer.zero_grad()                                                                             # :111
    loss.backward()
    if (cfg.SOLVER.CLIP_GRAD_VAL or cfg.SOLVER.CLIP_GRAD_L2NORM) and optim.fused_route(model, optimizer):
        # :116-126 as one multi-tensor pass (optimizer.FusedAdam / FusedSGD: clip, update, bf16 shadows; csrc/optim.hip)
        if cfg.SOLVER.CLIP_GRAD_VAL:
            optimizer.step_clipped(clip_value=cfg.SOLVER.CLIP_GRAD_VAL)
        else:
            optimizer.step_clipped(max_norm=cfg.SOLVER.CLIP_GRAD_L2NORM)
        return loss, mse, cross_entropy, recon, attns, tau
    if cfg.SOLVER.CLIP_GRAD_VAL:                                                                      # :116-123
        torch.nn.utils.clip_grad_value_(model.parameters(), cfg.SOLVER.CLIP_GRAD_VAL)
    elif cfg.SOLVER.CLIP_GRAD_L2NORM:
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.SOLVER.CLIP_GRAD_L2NORM)
    optimizer.step()                                                                                  # :126
    return loss, mse, cross_entropy, recon, attns, tau


def _slot_model(model):
    return model.module if hasattr(model, "module") else model          # DistributedDataParallel (:148)


@torch.no_grad()
def slot_recon_video(model, video, recon, attn, N=8):
    """The picture of steve_train_net.py:147-150 / :415-422 from the last batch of a loop: the autoregressive generation of
    video[:N] (reconstruct_autoregressive: cached keys and values on the decode kernel), then utils/slot_misc.visualize_slots
    on the raw attention `attn` [B,T,He*We,K] -> uint8 frames [1,T,3,Hg,Wg], the bytes add_video would make of the reference's
    fp32 frames.  The generation runs in eval mode and the mode is put back afterwards: the reference generates in whatever
    mode the loop left, i.e. after training with the decoder's dropout live."""
    from .slowfast.utils import slot_misc
    m = _slot_model(model)
    was_training = m.training
    m.eval()
    try:
        gen_video = m.reconstruct_autoregressive(video[:N])
    finally:
        m.train(was_training)
    He, We = m.slot_grid
    return slot_misc.visualize_slots(video.contiguous(), recon.contiguous(), gen_video.contiguous(), attn.contiguous(),
                                     (He, We), N=N, out_dtype=torch.uint8)


def slot_train_epoch(train_loader, model, optimizer, scaler, train_meter, cur_epoch, cfg, writer=None):
    """tools/steve_train_net.py:33-160 with the reference's argument list (scaler and train_meter are accepted and unused:
    bf16 needs no loss scaling, and the reference never touches the meter either).  `train_loader` yields video tensors
    [B,T,C,H,W]; `writer`, if given, receives the same scalar dict through add_scalars(dict, global_step=...).
    Returns {'tau', 'global_step'} like the reference (:153-158).  The steps run with raw_attns=True: the overlays are
    not made per step.  At the end of the epoch (:146-150) a writer that has add_video receives slot_recon_video of the last
    batch -- uint8 frames where the reference hands over fp32 ones that TensorBoard converts -- under
    tag='TRAIN_recons/epoch=%d' % (cur_epoch + 1); a writer without add_video gets the scalars alone."""
    model.train()
    data_size = len(train_loader)
    tau, global_step = None, cur_epoch * data_size
    video = recon = attn = None
    for cur_iter, video in enumerate(train_loader):
        global_step = cur_epoch * data_size + cur_iter
        if cfg.NUM_GPUS:
            video = video.cuda(non_blocking=True)
        loss, mse, ce, recon, attn, tau = slot_train_step(model, optimizer, video, global_step, cfg, raw_attns=True)
        recon = recon.detach()                                    # kept for the picture: not the step's autograd graph
        if writer is not None:
            with torch.no_grad():
                writer.add_scalars({"TRAIN/loss": loss.item(), "TRAIN/cross_entropy": ce.item(), "TRAIN/mse": mse.item(),
                                    "TRAIN/tau": tau, "TRAIN/lr_dvae": optimizer.param_groups[0]["lr"],
                                    "TRAIN/lr_enc": optimizer.param_groups[1]["lr"],
                                    "TRAIN/lr_dec": optimizer.param_groups[2]["lr"]}, global_step=global_step)
    if video is not None and hasattr(writer, "add_video"):                                            # :146-150
        frames = slot_recon_video(model, video, recon, attn)
        writer.add_video(frames, tag="TRAIN_recons/epoch=%d" % (cur_epoch + 1), global_step=cur_epoch + 1)
    return {"tau": tau, "global_step": global_step}


@torch.no_grad()
def slot_val_epoch(val_loader, model, cur_epoch, cfg, opd, writer=None):
    """The STEVE validation loop (tools/steve_train_net.py:161-212, eval_epoch there): eval mode, no gradients, every batch
    of `val_loader` (video tensors [B,T,C,H,W]) through the forward at opd['tau'].  The per-batch means of mse and
    cross_entropy go into a meters.StepStats on the device -- one launch per batch where the reference makes two .item()
    round trips -- and are read once at the end: val_loss = mean(mse) + mean(cross_entropy) over the batches, the double
    sums of the reference's MetricTracker.  Returns (val_loss, {'video', 'recon', 'attns'}) of the last batch, with the raw
    attention [B,T,N,K] for `attns` (slot_recon_video draws the VAL_recons picture of :415-422 from it); `writer`, if given,
    receives VAL/loss, VAL/cross_entropy and VAL/mse through add_scalars(dict, global_step=cur_epoch + 1).  A NaN loss
    raises at the read, as in the training loop (the reference returns the NaN)."""
    from .slowfast.utils import meters
    model.eval()
    dev = next(model.parameters()).device
    stats = video = recon = attns = None
    for video in val_loader:
        video = video.to(dev, non_blocking=True) if cfg.NUM_GPUS else video
        recon, cross_entropy, mse, attns = model(video, opd["tau"], cfg.SLOTS.HARD, attns="raw")      # :186
        mse, cross_entropy = mse.mean(), cross_entropy.mean()                                         # :189-190
        if stats is None:
            stats = meters.StepStats(video.device, ks=(), aux_names=("mse", "cross_entropy"))
        stats.update(None, None, mse + cross_entropy, (mse, cross_entropy), batch=video.shape[0])
    if stats is None:
        raise ValueError("slot_val_epoch: the loader is empty")
    fig = stats.read(reduce=False)                                # the reference averages per rank: no collective here
    val_loss = fig["mse"] + fig["cross_entropy"]                                                      # :197
    if writer is not None:
        writer.add_scalars({"VAL/loss": val_loss, "VAL/cross_entropy": fig["cross_entropy"], "VAL/mse": fig["mse"]},
                           global_step=cur_epoch + 1)                                                 # :204-208
    return val_loss, {"video": video, "recon": recon, "attns": attns}


@torch.no_grad()
def slot_eval_epoch(eval_loader, model, cfg=None):
    """FG-ARI evaluation of STEVE (tools/steve_eval_net.py:75-132): `eval_loader` yields (video [B,T,C,H,W], true_masks
    [B,T,S,1,H,W] with segment 0 = background); the slots' attention masks of `model.encode` are scored against the
    foreground segments over the whole clip (pixels of all frames flattened together).  Returns (mean, std over batches)
    of 100 x ARI; the ARI itself is computed on the device (utils/metrics.evaluate_ari).
    On the GPU, with a model that has `segment`, the masks stay at the slot grid's resolution: model.segment's arg-max map
    and the truth go straight into the contingency tables (metrics.evaluate_ari_segments) -- the same integers, hence the
    same scores, without the upsampled masks, attns_vis and the float64 one-hot.  FOCUS_SLOT_EVAL_FUSED=0 keeps the
    encode + evaluate_ari path everywhere."""
    from .slowfast.utils import metrics
    model.eval()
    dev = next(model.parameters()).device
    fused = dev.type == "cuda" and hasattr(model, "segment") and os.environ.get("FOCUS_SLOT_EVAL_FUSED", "1") != "0"
    scores = []
    for video, true_masks in eval_loader:
        video = video.to(dev)
        if fused:
            state = torch.cuda.get_rng_state(dev)
            _, seg, _ = model.segment(video)                                              # [B,T,He,We]
            if video.shape[-2] % seg.shape[-2] == 0 and video.shape[-1] % seg.shape[-1] == 0:
                truth = true_masks.to(dev)
                if truth.dtype not in (torch.bool, torch.uint8):
                    truth = truth.to(torch.uint8)                                         # evaluate_ari's reading of the masks
                scores.append(100 * metrics.evaluate_ari_segments(truth, seg, model.num_slots))
                continue
            torch.cuda.set_rng_state(state, dev)                 # a slot grid that does not divide the frame: the path below
        _, _, pred_masks = model.encode(video)                                            # [B,T,K,1,H,W]
        scores.append(100 * metrics.evaluate_ari(true_masks.to(dev).permute(0, 2, 1, 3, 4, 5)[:, 1:].flatten(start_dim=2),
                                                 pred_masks.permute(0, 2, 1, 3, 4, 5).flatten(start_dim=2)))
    t = torch.tensor(scores, dtype=torch.float64)
    return float(t.mean()), float(t.std(unbiased=False)) if len(scores) > 1 else 0.0


@torch.no_grad()
def eval_epoch(val_loader, model, cfg, stats=None):
    """The validation loop (tools/train_net.py:311-470, the single-label and the epickitchens branch): eval mode, no
    gradients, `val_loader` yields (inputs, labels, _, meta).  Every batch is one meters.StepStats.update (made here when
    none is given) and nothing is read until the end: one read, then the epoch's figures -- top-k errors, or verb / noun /
    action accuracies -- over all samples (and ranks) are returned.
    Under cfg.DATA.MULTI_LABEL (:433-435, :475 and meters.py:743-747) the predictions and the multi-hot labels of every batch
    are copied into a meters.MultiLabelStats (`stats`, or one made here with room for len(val_loader.dataset) rows, else for
    batches x the first batch's rows) and its read -- {'map', 'samples'} -- is returned: one gather and one
    focus_average_precision call per epoch.
    Under cfg.DETECTION.ENABLE (:336-366) `stats` is the AVA meter (meters.AVAMeter, meters.DeviceAVAMeter, or the caller's):
    every batch's scores, meta["ori_boxes"] and meta["metadata"] go to its update_stats(preds, ori_boxes, metadata) -- on the
    host, for a DeviceAVAMeter on the device; the meter is returned, to be read with log_epoch_stats or finalize_metrics."""
    from .slowfast.utils import meters
    model.eval()
    dev = next(model.parameters()).device
    if cfg.DETECTION.ENABLE:
        if stats is None:
            raise ValueError("eval_epoch under DETECTION.ENABLE needs the meter (update_stats(preds, ori_boxes, metadata)) as `stats`")
        for inputs, _, _, meta in val_loader:
            _detection_update(model, inputs, meta, stats, dev)
        return stats
    if cfg.DATA.MULTI_LABEL:
        for inputs, labels, _, meta in val_loader:
            inputs = [x.to(dev) for x in inputs] if isinstance(inputs, (list, tuple)) else inputs.to(dev)
            meta = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in meta.items()}
            preds = model(inputs, meta)
            if isinstance(preds, tuple):
                preds = preds[0]
            if stats is None:
                rows = len(val_loader.dataset) if hasattr(val_loader, "dataset") else len(val_loader) * preds.shape[0]
                stats = meters.MultiLabelStats(dev, preds.shape[1], rows)
            stats.update(preds, labels)
        return stats.read() if stats is not None else {}
    ek = zero = None
    for inputs, labels, _, meta in val_loader:
        inputs = [x.to(dev) for x in inputs] if isinstance(inputs, (list, tuple)) else inputs.to(dev)
        meta = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in meta.items()}
        ek = isinstance(labels, dict) and cfg.TRAIN.DATASET == "epickitchens"                    # :372
        labels = {k: v.to(dev) for k, v in labels.items()} if isinstance(labels, dict) else labels.to(dev)
        if stats is None:
            stats = meters.StepStats(dev, multitask=ek)
        if zero is None:
            zero = torch.zeros((), device=dev)                                                  # the loop computes no loss
        preds = model(inputs, meta)
        extra_preds = None
        if isinstance(preds, tuple):
            preds, extra_preds = preds
        if ek:
            stats.update(extra_preds, labels, zero, (zero, zero))
        else:
            stats.update(preds, labels, zero)
    if stats is None:
        return {}
    stats.read()
    return stats.epoch_stats()


def _detection_update(model, inputs, meta, meter, dev):
    """One batch of the detection branch of the test and validation loops (test_net.py:55-77, train_net.py:336-366): scores of
    the boxes of meta["boxes"], copied to the host with meta["ori_boxes"] and meta["metadata"] for the meter.  The boxes go to
    the model as the loader made them, so that a batch index out of range is refused on the host.  A meters.DeviceAVAMeter
    receives the device tensors as they are and gathers the ranks once, when it is read; for any other meter the three tensors
    of every rank are gathered here with all_gather_unaligned, as the reference does (test_net.py:71-74)."""
    from .slowfast.utils import distributed as du
    from .slowfast.utils import meters
    inputs = [x.to(dev) for x in inputs] if isinstance(inputs, (list, tuple)) else inputs.to(dev)
    boxes = meta["boxes"]
    meta = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in meta.items()}
    preds = model(inputs, meta, bboxes=boxes)
    if isinstance(preds, tuple):
        preds = preds[0]
    if isinstance(meter, meters.DeviceAVAMeter):
        meter.update_stats(preds.detach(), meta["ori_boxes"].detach(), meta["metadata"].detach())
        return
    rows = [preds.detach().cpu(), meta["ori_boxes"].detach().cpu(), meta["metadata"].detach().cpu()]
    if du.get_world_size() > 1:
        rows = [torch.cat(du.all_gather_unaligned(t), dim=0) for t in rows]
    meter.update_stats(*rows)


def _takes_metadata(meter):
    import inspect
    try:
        return "metadata" in inspect.signature(meter.update_stats).parameters
    except (TypeError, ValueError, AttributeError):
        return False


@torch.no_grad()
def perform_test(test_loader, model, test_meter, cfg):
    """Multi-view testing (tools/test_net.py:24-157): every clip of every video goes through the
    model in eval mode (softmax scores), the meter sums the views per video.  `test_loader` yields
    (inputs, labels, video_idx, meta) like the reference's loaders.  Dict labels, or a meter whose update_stats takes
    `metadata` (meters.EPICTestMeter), take the epickitchens branch (:85-111): both heads and the narration ids go to the
    meter.  A meters.DeviceTestMeter receives device tensors as they are, without a copy to the host.
    Under cfg.DETECTION.ENABLE (:55-77) the model takes meta["boxes"] and the meter -- meters.AVAMeter, or any object with
    that method -- receives update_stats(preds, ori_boxes, metadata) on the host, a meters.DeviceAVAMeter on the device;
    finalize_metrics() is called if the meter has one (for the two AVA meters it returns the mAP@0.5IOU)."""
    from .slowfast.utils import meters
    model.eval()
    dev = next(model.parameters()).device
    if cfg is not None and cfg.DETECTION.ENABLE:
        for inputs, _, _, meta in test_loader:
            _detection_update(model, inputs, meta, test_meter, dev)
        return test_meter.finalize_metrics() if hasattr(test_meter, "finalize_metrics") else None
    ek_meter = _takes_metadata(test_meter)
    on_device = isinstance(test_meter, (meters.DeviceTestMeter, meters.EPICTestMeter))
    for inputs, labels, video_idx, meta in test_loader:
        inputs = [x.to(dev) for x in inputs] if isinstance(inputs, (list, tuple)) else inputs.to(dev)
        meta = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in meta.items()}
        preds = model(inputs, meta)
        if isinstance(labels, dict) or ek_meter:
            extra_preds = preds[1]
            distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size() > 1
            if distributed:
                raise NotImplementedError("the multi-rank gather of narration ids (test_net.py:87-98) is not part of this path")
            args = ((extra_preds["verb"], extra_preds["noun"]), (labels["verb"], labels["noun"]), meta, video_idx)
            if not on_device:
                args = (tuple(p.detach().cpu() for p in args[0]), tuple(l.detach().cpu() for l in args[1]), meta,
                        video_idx.detach().cpu())
            test_meter.update_stats(*args)
            continue
        if isinstance(preds, tuple):
            preds = preds[0]
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            from .slowfast.utils import distributed as du
            preds, labels, video_idx = du.all_gather([preds, labels.to(dev), video_idx.to(dev)])
        test_meter.update_stats(preds, labels, video_idx)
    if ek_meter:
        test_meter.finalize_metrics()
        return test_meter.stats
    return test_meter.finalize_metrics()


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors(o)


def live_autograd_tensors(device=None):
    """CUDA tensors that still hang on an autograd graph (grad_fn is not None), found through the garbage collector's
    object list: the outputs of an earlier forward that somebody still references."""
    import gc
    import warnings
    found = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # isinstance() on lazy module proxies (torch.distributed.reduce_op) warns
        for o in gc.get_objects():
            try:
                if isinstance(o, torch.Tensor) and o.is_cuda and o.grad_fn is not None and (device is None or o.device == device):
                    found.append(o)
            except Exception:       # objects in odd states while being torn down
                pass
    return found


class GraphedStep:
    """One HIP graph for a launch-bound step (the STEVE slot update issues ~2000 kernels of 3-30 us per step: the host,
    not the GPU, sets its eager time).  `fn` takes no arguments, reads its inputs from tensors that stay in place, and
    runs forward + backward (gradients it leaves in .grad are rewritten by every replay).  The class owns the warm-up
    runs (on a side stream, as torch.cuda.graphs requires) and drops their outputs; `replay()` re-issues the whole
    step with one launch.

    Failure this class guards against (gpurun_out/r2_b42.log: `Segmentation fault in torch/cuda/graphs.py capture_end`
    on ROCm 7.2): an output of an EARLIER run of the step that is still referenced keeps that run's autograd graph --
    and the buffers it saved -- alive across the capture, and ending the capture then crashes inside the HIP runtime.
    The cause sits with whoever holds the reference, so the guard sits here, before the capture starts: after the
    warm-up the collector runs, the device is synchronised, and if ANY CUDA tensor with a grad_fn is still reachable
    (the caller's outputs of an earlier eager step, or outputs `fn` stores somewhere itself) the constructor raises
    instead of capturing.  `allow_live` names tensors the caller knows about and vouches for."""

    def __init__(self, fn, warmup=2, reset=None, allow_live=()):
        """reset: called before every warm-up run and before the capture (e.g. set .grad to None, so that the captured
        backward ASSIGNS gradients instead of accumulating into tensors from outside the graph)."""
        import gc
        import weakref
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        refs = []
        with torch.cuda.stream(side):
            for _ in range(warmup):
                if reset is not None:
                    reset()
                out = fn()
                refs.extend(weakref.ref(t) for t in _tensors(out))
                del out
        cur.wait_stream(side)
        if reset is not None:
            reset()
        gc.collect()
        torch.cuda.synchronize()
        if any(r() is not None for r in refs):
            raise RuntimeError("GraphedStep: fn keeps its own outputs alive between calls (a warm-up output is still referenced "
                               "after `del`); capturing now would crash in hipStreamEndCapture")
        ok = {id(t) for t in allow_live}
        live = [t for t in live_autograd_tensors(torch.device("cuda", torch.cuda.current_device())) if id(t) not in ok]
        if live:
            def who(t):
                try:
                    return [type(r).__name__ + (":" + ",".join(k for k, v in r.items() if v is t)[:60] if isinstance(r, dict) else "")
                            for r in gc.get_referrers(t) if r is not live][:3]
                except Exception:
                    return []
            raise RuntimeError("GraphedStep: %d CUDA tensor(s) of an earlier forward are still referenced (shape, grad_fn, held by: "
                               "%s); their autograd graph would be alive across the capture (crash in hipStreamEndCapture on "
                               "ROCm 7.2).  Drop them (del / detach) before building the graph" %
                               (len(live), [(tuple(t.shape), type(t.grad_fn).__name__, who(t)) for t in live[:4]]))
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outputs = fn()

    def replay(self):
        self.graph.replay()
        return self.outputs


def synthetic_batch(cfg, batch, device, seed=0):
    """Synthetic clips of BASELINE.md section 3: frames ~ N(0,1) [B,3,T,H,W], boxes [B,T,O,4] cxcywh with
    cx,cy ~ U(0.3,0.7), w,h ~ U(0.1,0.5) kept inside the frame, one object slot emptied, labels ~ randint.
    Drawn with a CPU generator so every box/rank sees the same numbers for a given seed."""
    g = torch.Generator().manual_seed(seed)
    Tn, S, O = cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE, cfg.ORVIT.O
    x = torch.randn(batch, 3, Tn, S, S, generator=g)
    wh = 0.1 + 0.4 * torch.rand(batch, Tn, O, 2, generator=g)
    c = 0.3 + 0.4 * torch.rand(batch, Tn, O, 2, generator=g)
    c = torch.minimum(torch.maximum(c, wh / 2), 1 - wh / 2)
    boxes = torch.cat([c, wh], dim=-1)
    boxes[batch - 1, :, O - 1] = 0                                 # empty-box path
    if cfg.TRAIN.DATASET == "epickitchens":                        # verb (97) / noun (300) label dict (train_net.py:95)
        labels = {"verb": torch.randint(0, 97, (batch,), generator=g).to(device),
                  "noun": torch.randint(0, 300, (batch,), generator=g).to(device)}
    else:
        labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (batch,), generator=g).to(device)
    return [x.to(device)], labels, {"orvit_bboxes": boxes.to(device)}
