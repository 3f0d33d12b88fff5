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
