"""Multi-view test ensembling (mirror of the arithmetic of slowfast/utils/meters.py:235-410 `TestMeter`; its timers and
JSON logging are plumbing and are not reproduced).  Every video is sampled as NUM_ENSEMBLE_VIEWS x NUM_SPATIAL_CROPS
clips; clip i belongs to video i // num_clips; predictions are summed (or max-ed) per video and top-k accuracy is
taken over the videos.  With multi_label=True the labels are multi-hot rows and the metric is get_map (meters.py:1275-1299):
the mean over the classes of scikit-learn's average precision."""
import numpy as np
import torch

from . import metrics


def _average_precision_columns(scores, labels):
    """sklearn.metrics.average_precision_score(labels, scores, average=None) for binary columns, restated in numpy with
    scikit-learn's own arithmetic (_binary_clf_curve, precision_recall_curve, average_precision_score): per class a stable
    descending sort, one threshold per distinct score, AP = sum over thresholds of (recall step) x precision."""
    aps = np.zeros(scores.shape[1], dtype=np.float64)
    for c in range(scores.shape[1]):
        order = np.argsort(scores[:, c], kind="mergesort")[::-1]
        s, y = scores[order, c], labels[order, c] == 1
        idx = np.r_[np.where(np.diff(s))[0], y.size - 1]
        tps = np.cumsum(y, dtype=np.float64)[idx]
        fps = 1 + idx - tps
        ps = tps + fps
        precision = np.zeros_like(tps)
        np.divide(tps, ps, out=precision, where=(ps != 0))
        recall = tps / tps[-1]
        precision, recall = np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0))
        aps[c] = max(0.0, -np.sum(np.diff(recall) * precision[:-1]))
    return aps


def get_map(preds, labels):
    """meters.py:1275-1299: the mean average precision over the classes that have a positive; 0.0 where scikit-learn raises
    and the reference falls into its `except` (a score that is not finite, no class with a positive, an empty table).
    numpy arrays and CPU tensors are scored here on the host, without scikit-learn; tensors on the device by one
    focus_average_precision call and one small copy.  Labels other than 0 / 1 in a kept class raise ValueError: what
    scikit-learn makes of them depends on its version."""
    if isinstance(preds, torch.Tensor) and preds.is_cuda:
        from focus_amd import ops
        _, _, summary, flag = ops.average_precision(preds.detach().float(), labels.detach().to(preds.device, torch.float32))
        t = torch.cat([summary, flag.double()]).cpu()                         # the one copy to the host
        return _map_from(float(t[0]), int(t[2]))
    preds = preds.detach().numpy() if isinstance(preds, torch.Tensor) else np.asarray(preds)
    labels = labels.detach().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    keep = ~np.all(labels == 0, axis=0)
    preds, labels = preds[:, keep], labels[:, keep]
    if not np.all((labels == 0) | (labels == 1)):
        raise ValueError("get_map: labels are 0 or 1")
    if preds.shape[0] == 0 or preds.shape[1] == 0 or not np.all(np.isfinite(preds)):
        return np.mean([0])                                                    # the reference's `except ValueError` path
    return np.mean(_average_precision_columns(preds, labels))


def _map_from(mean_ap, flag):
    if flag & 1:
        raise ValueError("get_map: labels are 0 or 1")
    return np.mean([0]) if flag & 6 else np.float64(mean_ap)


class TestMeter(object):
    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=False, ensemble_method="sum"):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self.multi_label = multi_label
        self.ensemble_method = ensemble_method
        self.video_preds = torch.zeros((num_videos, num_cls))
        if multi_label:
            self.video_preds -= 1e10                            # meters.py:276-277
        self.video_labels = torch.zeros((num_videos, num_cls)) if multi_label else torch.zeros((num_videos)).long()
        self.clip_count = torch.zeros((num_videos)).long()
        self.stats = {}

    def reset(self):
        self.clip_count.zero_()
        self.video_preds.zero_()
        if self.multi_label:
            self.video_preds -= 1e10
        self.video_labels.zero_()

    def update_stats(self, preds, labels, clip_ids):
        """meters.py:300-332, vectorised: one index_add_ / index_reduce_ per batch instead of a Python loop per clip.  The
        multi-label form keeps the reference's loop: its table starts at -1e10, where the order of the fp32 sums shows."""
        if self.multi_label:
            preds, labels = preds.detach().float().cpu(), labels.detach().float().cpu()
            for ind, cid in enumerate(clip_ids.detach().cpu().tolist()):
                vid_id = int(cid) // self.num_clips
                if self.video_labels[vid_id].sum() > 0:
                    assert torch.equal(self.video_labels[vid_id], labels[ind]), "clips of one video disagree on its labels"
                self.video_labels[vid_id] = labels[ind]
                if self.ensemble_method == "sum":
                    self.video_preds[vid_id] += preds[ind]
                else:
                    self.video_preds[vid_id] = torch.max(self.video_preds[vid_id], preds[ind])
                self.clip_count[vid_id] += 1
            return
        preds, labels = preds.detach().float().cpu(), labels.detach().cpu().long()
        vid = (clip_ids.detach().cpu().long() // self.num_clips)
        seen = self.video_labels[vid] > 0
        assert torch.equal(self.video_labels[vid][seen], labels[seen]), "clips of one video disagree on its label"
        self.video_labels[vid] = labels
        if self.ensemble_method == "sum":
            self.video_preds.index_add_(0, vid, preds)
        else:
            self.video_preds.index_reduce_(0, vid, preds, "amax", include_self=True)
        self.clip_count.index_add_(0, vid, torch.ones_like(vid))

    def finalize_metrics(self, ks=(1, 5)):
        """meters.py:372-410 -> {'split': 'test_final', 'top1_acc': 'xx.xx', ...}, or with multi_label {'split', 'map'};
        `complete` says whether every video received exactly num_clips clips (the reference only logs a warning)."""
        self.stats = {"split": "test_final", "complete": bool(torch.all(self.clip_count == self.num_clips))}
        if self.multi_label:
            self.stats["map"] = get_map(self.video_preds.cpu().numpy(), self.video_labels.cpu().numpy())
            return self.stats
        correct = metrics.topks_correct(self.video_preds, self.video_labels, ks)
        for k, x in zip(ks, correct):
            self.stats["top{}_acc".format(k)] = "{:.{prec}f}".format(float(x / self.video_preds.size(0)) * 100.0, prec=2)
        return self.stats


# ---- statistics kept on the device (csrc/step_stats.hip) --------------------------------------------------------------------
_STEPS, _SAMPLES, _NAN, _NAN_STEP, _CORRECT = 0, 1, 2, 3, 4       # the int64 table of focus_topk_stats
_NI, _NF = 16, 8


def _distributed_world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class StepStats(object):
    """The per-step numbers of the training and validation loops (train_net.py:151-269, :372-467) -- top-k errors, or for
    EPIC-Kitchens verb / noun / action accuracies, the losses, and the NaN guard of misc.check_nan_losses -- accumulated by
    one kernel launch per step in two small device tables.  `update` never synchronises; `read` is the only sync: one
    all-reduce when there are several ranks, one small device-to-host copy, the window's figures, and the raise the
    reference makes in the step when a loss was NaN.  A window is what lies between two reads; every read also folds its
    window into host-side epoch totals (`epoch_stats`).

    ks=() keeps no top-k figures (STEVE: update(None, None, loss, (mse, cross_entropy), batch=B)); `aux_names` names the
    means of the aux losses in the figures (default: verb_loss, noun_loss when multitask)."""

    def __init__(self, device, ks=(1, 5), multitask=False, aux_names=None):
        self.ks = tuple(int(k) for k in ks)
        self.multitask = bool(multitask)
        self.aux_names = tuple(aux_names) if aux_names is not None else (("verb_loss", "noun_loss") if multitask else ())
        if len(self.ks) > 4 or len(self.aux_names) > 2:
            raise ValueError("StepStats keeps at most 4 ks and 2 aux losses; got %s, %s" % (self.ks, self.aux_names))
        self.acc_i = torch.zeros(_NI, dtype=torch.int64, device=device)
        self.acc_f = torch.zeros(_NF, dtype=torch.float64, device=device)
        self.reset_epoch()

    def reset_epoch(self):
        self._epoch = torch.zeros(_NI + _NF, dtype=torch.float64)
        self._steps_read = 0                                    # this rank's steps of the windows read so far

    def update(self, preds, labels, loss, aux_losses=(), batch=None):
        """One launch, no sync.  preds / labels: tensors, or for EPIC-Kitchens the {'verb','noun'} dicts; labels are class
        indices or the dense rows of mixup; loss and aux_losses are 0-d device tensors."""
        from focus_amd import ops
        if isinstance(labels, dict):
            preds, labels = (preds["verb"], preds["noun"]), (labels["verb"], labels["noun"])
        elif preds is None:
            preds, labels = (), ()
        losses = [l.detach().float().reshape(()) for l in (loss,) + tuple(aux_losses)]
        ops.topk_stats(self.acc_i, self.acc_f, tuple(p.detach() for p in _as_tuple(preds)), _as_tuple(labels),
                       self.ks or (1,), losses, batch=batch)

    def _figures(self, t, weighted):
        ints, fl = t[:_NI], t[_NI:]
        samples, steps = float(ints[_SAMPLES]), float(ints[_STEPS])
        out = {}
        pct = (lambda c: 100.0 * c / samples) if samples else (lambda c: float("nan"))
        for j, k in enumerate(self.ks):
            c = [float(ints[_CORRECT + 4 * h + j]) for h in range(3)]
            if self.multitask:
                out["verb_top%d_acc" % k], out["noun_top%d_acc" % k], out["action_top%d_acc" % k] = pct(c[0]), pct(c[1]), pct(c[2])
            else:
                out["top%d_err" % k] = pct(samples - c[0])
        den = samples if weighted else steps
        for i, name in enumerate(("loss",) + self.aux_names):
            out[name] = float(fl[(3 if weighted else 0) + i]) / den if den else float("nan")
        out["samples"] = int(samples)
        return out

    def read(self, reset=True, reduce=True):
        """The window's figures.  Plain: top{k}_err, loss; EK: verb_/noun_/action_top{k}_acc, verb_loss, noun_loss, loss; both:
        samples (over all ranks) and steps.  Percentages are 100 * count / samples, losses the mean over steps (and ranks).
        Raises RuntimeError("ERROR: Got NaN losses ...") when a NaN loss was latched on any rank; by then the failing
        step's update has been applied, and the window is reset as asked."""
        t = torch.cat([self.acc_i.double(), self.acc_f])                      # counts are far below 2^53: exact in double
        world = _distributed_world() if reduce else 1
        if world > 1:
            import torch.distributed as dist
            own = t[:_NAN_STEP + 1].clone()                                   # this rank's steps and NaN step
            dist.all_reduce(t)                                                # sums; the NaN flag becomes a count of ranks
            t = torch.cat([t, own])
        t = t.cpu()                                                           # the one copy to the host
        t, own = t[:_NI + _NF], t[_NI + _NF:] if world > 1 else t
        if reset:
            self.acc_i.zero_()
            self.acc_f.zero_()
        nan_here = own[_NAN] > 0
        nan_step = self._steps_read + int(own[_NAN_STEP])
        if reset:
            self._steps_read += int(own[_STEPS])
            self._epoch += t
        if t[_NAN] > 0:
            raise RuntimeError("ERROR: Got NaN losses (step %d)" % nan_step if nan_here else
                               "ERROR: Got NaN losses (on another rank)")
        out = self._figures(t, weighted=False)
        out["steps"] = int(t[_STEPS]) // world
        return out

    def epoch_stats(self):
        """The totals of the windows read (and reset) so far, the way TrainMeter / EPICTrainMeter.log_epoch_stats report them:
        errors and accuracies from the counts, losses weighted by the batch size."""
        out = self._figures(self._epoch, weighted=True)
        out["steps"] = self._steps_read
        return out


def _as_tuple(x):
    return (x,) if isinstance(x, torch.Tensor) else tuple(x)


class DeviceTestMeter(object):
    """TestMeter with its tables on the device: `update_stats` is one focus_view_accumulate launch and no sync (CPU clip_ids
    and labels are copied non-blocking), `finalize_metrics` scores the table with focus_topk_stats.  The assertion
    TestMeter makes per batch -- the clips of a video agree on its label -- is deferred to finalize_metrics.
    multi_label=True: the label table is float32 [num_videos,num_cls], the score table starts at -1e10, `update_stats` is one
    focus_view_accumulate_dense launch and `finalize_metrics` one focus_average_precision call and one copy -> 'map'."""

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, device, ensemble_method="sum", multi_label=False):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self.ensemble_method = ensemble_method
        self.multi_label = bool(multi_label)
        self.device = torch.device(device)
        self.video_preds = torch.zeros((num_videos, num_cls), device=self.device)
        if self.multi_label:
            self.video_preds -= 1e10
        self.video_labels = torch.zeros((num_videos, num_cls), device=self.device) if self.multi_label else \
            torch.zeros((num_videos), device=self.device).long()
        self.clip_count = torch.zeros((num_videos), device=self.device).long()
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stats = {}

    def reset(self):
        self.clip_count.zero_()
        self.video_preds.zero_()
        if self.multi_label:
            self.video_preds -= 1e10
        self.video_labels.zero_()
        self.flag.zero_()

    def update_stats(self, preds, labels, clip_ids):
        from focus_amd import ops
        if self.multi_label:
            labels = labels.detach().to(self.device, torch.float32, non_blocking=True)
            clip_ids = clip_ids.detach().to(self.device, torch.int64, non_blocking=True).contiguous()
            ops.view_accumulate_dense(preds.detach(), clip_ids, labels if labels.stride(-1) == 1 else labels.contiguous(),
                                      self.num_clips, self.video_preds, self.video_labels, self.clip_count, self.flag,
                                      self.ensemble_method)
            return
        labels = labels.detach().to(self.device, torch.int64, non_blocking=True).contiguous()
        clip_ids = clip_ids.detach().to(self.device, torch.int64, non_blocking=True).contiguous()
        ops.view_accumulate(preds.detach(), clip_ids, labels, self.num_clips, self.video_preds, self.video_labels,
                            self.clip_count, self.flag, self.ensemble_method)

    def _check_flag(self, flag):
        assert not flag & 1, "clips of one video disagree on its label"
        assert not flag & 2, "a clip id lies outside [0, num_videos * num_clips)"

    def finalize_metrics(self, ks=(1, 5)):
        from focus_amd import ops
        if self.multi_label:
            _, _, summary, ap_flag = ops.average_precision(self.video_preds, self.video_labels)
            complete = (self.clip_count == self.num_clips).all().double().reshape(1)
            t = torch.cat([summary, ap_flag.double(), complete, self.flag.double()]).cpu()   # the one copy to the host
            self._check_flag(int(t[4]))
            self.stats = {"split": "test_final", "complete": bool(t[3]), "map": _map_from(float(t[0]), int(t[2]))}
            return self.stats
        acc_i = torch.zeros(_NI, dtype=torch.int64, device=self.device)
        acc_f = torch.zeros(_NF, dtype=torch.float64, device=self.device)
        ops.topk_stats(acc_i, acc_f, self.video_preds, self.video_labels, ks)
        complete = (self.clip_count == self.num_clips).all().to(torch.int64).reshape(1)
        t = torch.cat([acc_i, complete, self.flag.to(torch.int64)]).cpu()     # the one copy to the host
        self._check_flag(int(t[_NI + 1]))
        self.stats = {"split": "test_final", "complete": bool(t[_NI])}
        n = self.video_preds.size(0)
        for j, k in enumerate(ks):
            x = torch.tensor(float(t[_CORRECT + j]))                           # the fp32 count metrics.topks_correct returns
            self.stats["top{}_acc".format(k)] = "{:.{prec}f}".format(float(x / n) * 100.0, prec=2)
        return self.stats


class MultiLabelStats(object):
    """What ValMeter.update_predictions and the epoch-end get_map do under DATA.MULTI_LABEL (meters.py:694-747,
    train_net.py:433-475), without the Python list of batches: `update` copies the batch into rows [offset, offset + n) of two
    preallocated float32 tables [capacity,num_cls] -- the offset is known on the host, nothing synchronises -- and `read`
    scores the filled part with get_map.  With several ranks `read` gathers the filled parts once; the reference gathers
    every batch.  CPU tables take the numpy path of get_map."""

    def __init__(self, device, num_cls, capacity):
        self.device = torch.device(device)
        self.preds = torch.empty((int(capacity), int(num_cls)), dtype=torch.float32, device=self.device)
        self.labels = torch.empty((int(capacity), int(num_cls)), dtype=torch.float32, device=self.device)
        self.offset = 0

    def reset(self):
        self.offset = 0

    def update(self, preds, labels):
        n = preds.shape[0]
        if self.offset + n > self.preds.shape[0]:
            raise RuntimeError("MultiLabelStats: %d rows do not fit behind %d of a capacity of %d" % (
                n, self.offset, self.preds.shape[0]))
        self.preds[self.offset:self.offset + n].copy_(preds.detach(), non_blocking=True)
        self.labels[self.offset:self.offset + n].copy_(labels.detach(), non_blocking=True)
        self.offset += n

    def read(self, reset=True, reduce=True):
        """{'map': get_map over the rows of all ranks, 'samples': their number}."""
        preds, labels = self.preds[:self.offset], self.labels[:self.offset]
        world = _distributed_world() if reduce else 1
        if world > 1:
            import torch.distributed as dist
            counts = [torch.zeros(1, dtype=torch.int64, device=self.device) for _ in range(world)]
            dist.all_gather(counts, torch.tensor([self.offset], dtype=torch.int64, device=self.device))
            counts = [int(c) for c in torch.cat(counts).cpu()]
            both = torch.zeros((max(counts), 2 * self.preds.shape[1]), dtype=torch.float32, device=self.device)
            both[:self.offset] = torch.cat([preds, labels], dim=1)
            parts = [torch.empty_like(both) for _ in range(world)]
            dist.all_gather(parts, both)                                      # the one gather of the epoch
            both = torch.cat([p[:c] for p, c in zip(parts, counts)])
            preds, labels = both[:, :self.preds.shape[1]], both[:, self.preds.shape[1]:]
        out = {"map": float(get_map(preds, labels)), "samples": int(preds.shape[0])}
        if reset:
            self.reset()
        return out


def get_ava_mini_groundtruth(full_groundtruth):
    """meters.py:32-47: the ground truth of the key frames whose second is a multiple of 4, the subset the validation
    epochs are scored on unless AVA.FULL_TEST_ON_VAL."""
    from collections import defaultdict
    ret = [defaultdict(list), defaultdict(list), defaultdict(list)]
    for i in range(3):
        for key in full_groundtruth[i].keys():
            if int(key.split(",")[1]) % 4 == 0:
                ret[i][key] = full_groundtruth[i][key]
    return ret


class AVAMeter(object):
    """meters.py:50-232 without the timers and the JSON logger: the rows of an epoch are kept on the host and scored by
    ava_eval_helper.evaluate_ava at the end.  `mode` is 'train', 'val' or 'test'; 'test', and 'val' under
    AVA.FULL_TEST_ON_VAL, are scored on the whole ground truth, 'val' otherwise on the mini ground truth.  The reference
    writes detections_latest.csv and groundtruth_latest.csv on every evaluation; here only with write_csv=True."""

    def __init__(self, overall_iters, cfg, mode):
        import os
        from collections import deque
        from . import ava_eval_helper
        from ..datasets import ava_helper
        if mode not in ("train", "val", "test"):
            raise NotImplementedError("Unknown mode: {}".format(mode))
        self.cfg = cfg
        self.lr = None
        self.loss = deque(maxlen=int(cfg.LOG_PERIOD))
        self.full_ava_test = cfg.AVA.FULL_TEST_ON_VAL
        self.mode = mode
        self.overall_iters = overall_iters
        self.full_map = None
        self.excluded_keys = ava_eval_helper.read_exclusions(os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.EXCLUSION_FILE))
        self.categories, self.class_whitelist = ava_eval_helper.read_labelmap(
            os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.LABEL_MAP_FILE))
        self.full_groundtruth = ava_eval_helper.read_csv(os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.GROUNDTRUTH_FILE),
                                                         self.class_whitelist)
        self.mini_groundtruth = get_ava_mini_groundtruth(self.full_groundtruth)
        _, self.video_idx_to_name = ava_helper.load_image_lists(cfg, mode == "train")
        self.output_dir = cfg.OUTPUT_DIR
        self.reset()

    def _groundtruth(self):
        full = self.mode == "test" or (self.full_ava_test and self.mode == "val")
        return self.full_groundtruth if full else self.mini_groundtruth

    def reset(self):
        self.loss.clear()
        self.all_preds, self.all_ori_boxes, self.all_metadata = [], [], []

    def update_stats(self, preds, ori_boxes, metadata, loss=None, lr=None):
        """preds [n,C] scores, ori_boxes [n,5] (batch index, x1, y1, x2, y2), metadata [n,2] (video index, second); kept in
        'val' and 'test' mode only, as in the reference."""
        if self.mode in ["val", "test"]:
            self.all_preds.append(preds)
            self.all_ori_boxes.append(ori_boxes)
            self.all_metadata.append(metadata)
        if loss is not None:
            self.loss.append(float(loss))
        if lr is not None:
            self.lr = lr

    def _rows(self):
        if not self.all_preds:
            raise RuntimeError("AVAMeter.finalize_metrics: no rows were received (mode %r keeps %s)" % (
                self.mode, "rows" if self.mode in ("val", "test") else "none"))
        return torch.cat(self.all_preds, dim=0), torch.cat(self.all_ori_boxes, dim=0), torch.cat(self.all_metadata, dim=0)

    def finalize_metrics(self, log=True, write_csv=False):
        """-> self.full_map, the mAP@0.5IOU over the rows received since the last reset."""
        from . import ava_eval_helper
        preds, ori_boxes, metadata = self._rows()
        self.full_map = ava_eval_helper.evaluate_ava(preds, ori_boxes, metadata, self.excluded_keys, self.class_whitelist,
                                                     self.categories, groundtruth=self._groundtruth(),
                                                     video_idx_to_name=self.video_idx_to_name, write_csv=write_csv)
        if log:
            _ava_log({"mode": self.mode, "map": self.full_map})
        return self.full_map

    def log_epoch_stats(self, cur_epoch):
        """The epoch's record ({'_type', 'cur_epoch', 'mode', 'map'}) in 'val' and 'test' mode; None in 'train' mode."""
        if self.mode not in ["val", "test"]:
            return None
        self.finalize_metrics(log=False)
        stats = {"_type": "{}_epoch".format(self.mode), "cur_epoch": "{}".format(cur_epoch + 1), "mode": self.mode,
                 "map": self.full_map}
        _ava_log(stats)
        return stats


def _ava_log(stats):
    import logging
    logging.getLogger(__name__).info("json_stats: %s", stats)


class DeviceAVAMeter(AVAMeter):
    """AVAMeter with the evaluation on the device (csrc/ava_eval.hip).  At construction the ground truth in use is uploaded
    once: a dense (video index, second) -> image lookup (-1 no ground truth, -2 excluded), the ground-truth rows by image
    (class ids, float64 boxes) and the rows per class.  `update_stats` keeps the device tensors it is given and does not
    synchronise.  `finalize_metrics` groups the rows by image with one stable sort, runs focus_ava_match and focus_voc_ap,
    makes one small copy to the host -- its only sync -- and raises for a set flag.  `self.ap` is the per-class table
    (float64 [C] on the device, NaN without ground truth).  Equal scores within a class are ordered by descending row of
    the concatenated update_stats calls, like the host meter.  With several ranks every rank's rows are gathered once, in
    finalize_metrics (a length gather and one padded all_gather), rank after rank."""

    def __init__(self, overall_iters, cfg, mode, device="cuda"):
        super().__init__(overall_iters, cfg, mode)
        import numpy as np
        self.device = torch.device(device)
        self.ap = None
        gt = self._groundtruth()
        keys = [k for k in gt[0] if k not in self.excluded_keys]
        ids = [c["id"] for c in self.categories]
        if not ids or min(ids) < 1:
            raise ValueError("Classes should be 1-indexed.")
        self.num_classes = max(ids)
        gt_off, gt_class, gt_boxes = [0], [], []
        for k in keys:
            for b, l in zip(gt[0][k], gt[1][k]):
                gt_class.append(int(l))
                gt_boxes.append([b[1], b[0], b[3], b[2]])       # the reader's [y1, x1, y2, x2] -> (x1, y1, x2, y2)
            gt_off.append(len(gt_class))
        gt_class = np.asarray(gt_class, dtype=np.int32).reshape(-1)
        if gt_class.size and (gt_class.min() < 1 or gt_class.max() > self.num_classes):
            raise ValueError("DeviceAVAMeter: a ground-truth class id lies outside 1..%d" % self.num_classes)
        n_gt = np.bincount(gt_class - 1, minlength=self.num_classes).astype(np.int64)
        self.total_gt = int(n_gt.sum())
        video_of = {name: i for i, name in enumerate(self.video_idx_to_name)}
        split = lambda k: (k.rsplit(",", 1)[0], int(k.rsplit(",", 1)[1]))
        secs = [split(k)[1] for k in list(keys) + list(self.excluded_keys) if split(k)[0] in video_of]
        self._secs = max(secs) + 1 if secs else 1
        lookup = np.full((max(len(video_of), 1), self._secs), -1, dtype=np.int64)
        for i, k in enumerate(keys):
            name, sec = split(k)
            if name in video_of and sec >= 0:
                lookup[video_of[name], sec] = i
        for k in self.excluded_keys:
            name, sec = split(k)
            if name in video_of and sec >= 0:
                lookup[video_of[name], sec] = -2
        dev = self.device
        self._lookup = torch.from_numpy(lookup).to(dev)
        self._gt_off = torch.tensor(gt_off, dtype=torch.int64, device=dev)
        self._gt_class = torch.from_numpy(gt_class).to(dev)
        self._gt_boxes = torch.tensor(gt_boxes, dtype=torch.float64, device=dev).reshape(len(gt_boxes), 4)
        self._n_gt = torch.from_numpy(n_gt).to(dev)

    def update_stats(self, preds, ori_boxes, metadata, loss=None, lr=None):
        """Device tensors are kept as they are; host tensors are copied over without blocking.  `loss` is kept as given (a
        0-d device tensor is not read here)."""
        if self.mode in ["val", "test"]:
            self.all_preds.append(preds.detach().to(self.device, non_blocking=True))
            self.all_ori_boxes.append(ori_boxes.detach().to(self.device, non_blocking=True))
            self.all_metadata.append(metadata.detach().to(self.device, non_blocking=True))
        if loss is not None:
            self.loss.append(loss)
        if lr is not None:
            self.lr = lr

    def _gathered(self):
        preds, ori_boxes, metadata = self._rows()
        world = _distributed_world()
        if world == 1:
            return preds, ori_boxes, metadata
        import torch.distributed as dist
        C = preds.shape[1]
        both = torch.cat([preds.double(), ori_boxes.double().reshape(-1, 5), metadata.double().reshape(preds.shape[0], -1)[:, :2]],
                         dim=1)                                                # fp32 and bf16 values are exact in double
        counts = [torch.zeros(1, dtype=torch.int64, device=self.device) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([both.shape[0]], dtype=torch.int64, device=self.device))
        counts = [int(c) for c in torch.cat(counts).cpu()]
        padded = torch.zeros((max(counts), both.shape[1]), dtype=torch.float64, device=self.device)
        padded[:both.shape[0]] = both
        parts = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded)                                        # the one gather of the epoch
        both = torch.cat([p[:c] for p, c in zip(parts, counts)])
        return both[:, :C].to(preds.dtype), both[:, C:C + 5].float(), both[:, C + 5:]

    def finalize_metrics(self, log=True, write_csv=False):
        from focus_amd import ops
        if write_csv:
            raise NotImplementedError("DeviceAVAMeter writes no CSV files: score the epoch with AVAMeter(write_csv=True)")
        preds, ori_boxes, metadata = self._gathered()
        K, C = preds.shape
        if C < self.num_classes:
            raise ValueError("DeviceAVAMeter: %d score columns for class ids up to %d" % (C, self.num_classes))
        if preds.dtype not in (torch.float32, torch.bfloat16):
            preds = preds.float()
        preds = preds.contiguous()
        dev = self.device
        boxes = ori_boxes.reshape(K, 5)[:, 1:5].float().contiguous()
        metadata = metadata.reshape(K, -1).double()
        vid, sec = torch.round(metadata[:, 0]).long(), torch.round(metadata[:, 1]).long()
        V, S = self._lookup.shape
        inside = (vid >= 0) & (vid < V) & (sec >= 0) & (sec < S)
        image = torch.where(inside, self._lookup[vid.clamp(0, V - 1), sec.clamp(0, S - 1)], torch.full_like(vid, -1))
        # 1. group by image: one stable sort of the rows by (video, second); the rows of excluded images go to the end and
        #    belong to no group.  The number of groups stays on the device: K groups are passed, the surplus is empty.
        last = torch.iinfo(torch.int64).max
        key = torch.where(image == -2, torch.full_like(vid, last), vid * (1 << 32) + (sec & 0xFFFFFFFF))
        skey, det_rows = torch.sort(key, stable=True)
        first = torch.ones(K, dtype=torch.bool, device=dev)
        first[1:] = skey[1:] != skey[:-1]
        gid = torch.cumsum(first.long(), 0) - 1
        slot = torch.where(first, gid, torch.full_like(gid, K + 1))           # rows that open no group write to a spare slot
        end = (image != -2).sum().reshape(1)                                  # where the excluded rows begin
        grp_off = end.expand(K + 2).clone()                                   # the group they open there is empty, like the surplus
        grp_off.scatter_(0, slot, torch.arange(K, device=dev))
        grp_off = grp_off[:K + 1].contiguous()
        grp_image = torch.full((K + 2,), -1, dtype=torch.int64, device=dev)
        grp_image.scatter_(0, slot, image[det_rows])
        whitelist = torch.zeros(C, dtype=torch.uint8, device=dev)
        ids = [c - 1 for c in self.class_whitelist if 1 <= c <= self.num_classes]
        whitelist[torch.tensor(ids, dtype=torch.int64, device=dev)] = 1
        n_gt = torch.zeros(C, dtype=torch.int64, device=dev)
        n_gt[:self.num_classes] = self._n_gt
        # 2. the match, 3. the average precision
        self.bytes, self.counts, mflag = ops.ava_match(boxes, C, grp_off, det_rows.contiguous(), grp_image[:K].contiguous(),
                                                       self._gt_off, self._gt_class, self._gt_boxes, whitelist)
        self.ap, summary, vflag = ops.voc_average_precision(preds, self.bytes, n_gt, self.total_gt)
        t = torch.cat([summary, mflag.double(), vflag.double()]).cpu()        # 4. the one copy to the host
        mflag, vflag = int(t[2]), int(t[3])                                   # 5. the flags
        if mflag & ops.AVA_GT_OVERFLOW:
            raise RuntimeError("DeviceAVAMeter: an image has more than %d ground-truth rows of one class" % ops.AVA_GT_CAP)
        if mflag & ops.AVA_BAD_INDEX:
            raise RuntimeError("DeviceAVAMeter: the group tables are inconsistent")
        if vflag & ops.VOC_BAD_SCORE:
            raise ValueError("DeviceAVAMeter: a detection score is not finite")
        if vflag & (ops.VOC_TP_ABOVE_GT | ops.VOC_GT_ABOVE_TOTAL):
            raise ValueError("Number of true positives must be smaller than num_gt.")
        self.full_map = float(t[0])
        if log:
            _ava_log({"mode": self.mode, "map": self.full_map})
        return self.full_map


class EPICTestMeter(object):
    """meters.py:1134-1273 with the two tables on the device: two focus_view_accumulate launches per batch; the narration ids
    stay on the host, indexed from the host clip_ids."""

    def __init__(self, num_videos, num_clips, num_cls=(97, 300), overall_iters=0, device="cuda"):
        import numpy as np
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self.device = torch.device(device)
        self.verb_video_preds = torch.zeros((num_videos, num_cls[0]), device=self.device)
        self.noun_video_preds = torch.zeros((num_videos, num_cls[1]), device=self.device)
        self.verb_video_labels = torch.zeros((num_videos), device=self.device).long()
        self.noun_video_labels = torch.zeros((num_videos), device=self.device).long()
        self.metadata = np.zeros(num_videos, dtype=object)
        self.clip_count = torch.zeros((num_videos), device=self.device).long()
        self._noun_count = torch.zeros((num_videos), device=self.device).long()
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stats = {}

    def reset(self):
        for t in (self.clip_count, self._noun_count, self.verb_video_preds, self.verb_video_labels, self.noun_video_preds,
                  self.noun_video_labels, self.flag):
            t.zero_()
        self.metadata.fill(0)

    def update_stats(self, preds, labels, metadata, clip_ids):
        from focus_amd import ops
        host_ids = clip_ids.detach().cpu() if not clip_ids.is_cuda else None
        ids = clip_ids.detach().to(self.device, torch.int64, non_blocking=True).contiguous()
        for p, l, table, tl, cnt in ((preds[0], labels[0], self.verb_video_preds, self.verb_video_labels, self.clip_count),
                                     (preds[1], labels[1], self.noun_video_preds, self.noun_video_labels, self._noun_count)):
            l = l.detach().to(self.device, torch.int64, non_blocking=True).contiguous()
            ops.view_accumulate(p.detach(), ids, l, self.num_clips, table, tl, cnt, self.flag, "sum")
        if host_ids is None:
            host_ids = clip_ids.detach().cpu()                  # ids that only exist on the device: the one sync of this path
        for ind, cid in enumerate(host_ids.tolist()):
            if 0 <= cid < self.metadata.shape[0] * self.num_clips:
                self.metadata[int(cid) // self.num_clips] = metadata["narration_id"][ind]

    def finalize_metrics(self, ks=(1, 5)):
        from focus_amd import ops
        acc_i = torch.zeros(_NI, dtype=torch.int64, device=self.device)
        acc_f = torch.zeros(_NF, dtype=torch.float64, device=self.device)
        ops.topk_stats(acc_i, acc_f, (self.verb_video_preds, self.noun_video_preds),
                       (self.verb_video_labels, self.noun_video_labels), ks)
        t = torch.cat([acc_i, self.flag.to(torch.int64)]).cpu()
        assert not int(t[_NI]) & 2, "a clip id lies outside [0, num_videos * num_clips)"
        n = self.verb_video_preds.size(0)
        stats = {"split": "test_final"}
        for h, name in enumerate(("verb", "noun", "action")):
            for j, k in enumerate(ks):
                x = torch.tensor(float(t[_CORRECT + 4 * h + j]))
                stats["{}_top{}_acc".format(name, k)] = "{:.{prec}f}".format(float((x / n) * 100.0), prec=2)
        self.stats = stats
        return (self.verb_video_preds.cpu().numpy().copy(), self.noun_video_preds.cpu().numpy().copy()), \
               (self.verb_video_labels.cpu().numpy().copy(), self.noun_video_labels.cpu().numpy().copy()), \
               self.metadata.copy()
