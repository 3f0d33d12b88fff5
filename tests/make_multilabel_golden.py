"""TEST INFRASTRUCTURE: writes tests/golden/multilabel.npz from the reference's own slowfast/utils/meters.py, loaded as a
single file (its module-level imports of fvcore and of the reference's other modules are satisfied by stubs: get_map and
TestMeter use numpy, torch, scikit-learn and a Timer that only has to exist).  Runs only where the reference tree and
scikit-learn are present:
    python tests/make_multilabel_golden.py
The fixture is data only, three sets of records.
  ap.<case>.{scores, labels, map[, aps]}   small tables and what the reference's get_map returned for them (aps: what
      scikit-learn's average_precision_score(average=None) gave for the kept columns, where it does not raise).
  tm.<mode>.{preds, labels, clip_ids, splits, video_preds, video_labels, clip_count, map}   a TestMeter(multi_label=True) run
      whose clips arrive shuffled and split unevenly over batches, ensemble "max" and "sum".
  bce.{x, y, p, yp} and bce.<logit|prob>.<f64|f32>.{mean, sum, grad_mean, grad_sum}   nn.BCEWithLogitsLoss and nn.BCELoss of torch
      on the CPU, in float64 (inputs widened from fp32) and float32."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "multilabel.npz")


def _stub(name, **attrs):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        full = ".".join(parts[:i])
        if full not in sys.modules:
            sys.modules[full] = types.ModuleType(full)
        if i > 1:
            setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], sys.modules[full])
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference():
    import logging
    from oracle._ref_loader import REF

    class Timer(object):
        def reset(self):
            pass
    _stub("fvcore.common.timer", Timer=Timer)
    _stub("slowfast.datasets.ava_helper")
    _stub("slowfast.utils.logging", get_logger=logging.getLogger, log_json_stats=lambda stats: None)
    _stub("slowfast.utils.metrics")
    _stub("slowfast.utils.misc")
    _stub("slowfast.utils.ava_eval_helper", evaluate_ava=None, read_csv=None, read_exclusions=None, read_labelmap=None)
    _stub("slowfast.models.losses")
    spec = importlib.util.spec_from_file_location("_reference_meters", os.path.join(REF, "slowfast", "utils", "meters.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ap_cases():
    g = np.random.RandomState(7)

    def table(N, C, p=0.3, levels=None):
        s = g.randn(N, C).astype(np.float32)
        if levels:
            s = g.choice(np.float32(levels), size=(N, C)).astype(np.float32)
        return s, (g.rand(N, C) < p).astype(np.float32)
    out = {}
    out["ties"] = table(97, 5, levels=(-0.5, 0.25, 2.0))
    s, y = table(64, 4)
    y[:, 2] = 0
    out["zero_class"] = (s, y)
    s, y = table(65, 3)
    y[:, 0] = 1
    out["one_class"] = (s, y)
    s, y = table(40, 3)
    y[:, 0] = 0
    y[:, 2] = 0
    out["single_kept"] = (s, y)
    s, y = table(50, 4, levels=(0.125, 0.5, 0.75, 0.875))
    s[g.permutation(50)[:10]] = np.float32(-1e10)                             # videos the meter never saw
    out["fill"] = (s, y)
    s, y = table(33, 3)
    y[5, 1] = 1
    s[5, 1] = np.nan
    out["nan"] = (s, y)
    s, y = table(20, 3)
    out["none_kept"] = (s, np.zeros_like(y))
    out["random300"] = table(300, 8, p=0.2)                                  # more than one tile of 256 rows
    out["all_equal"] = (np.full((70, 2), 0.5, dtype=np.float32), table(70, 2)[1])
    return out


def test_meter_run(ref, mode):
    g = np.random.RandomState(11)
    nv, nc, C = 6, 3, 5
    video_labels = (g.rand(nv, C) < 0.4).astype(np.float32)
    video_labels[0] = 0
    video_labels[0, 3] = 1
    video_labels[4] = 0                                                       # a video without any label: never "seen"
    clip_ids = g.permutation(nv * nc).astype(np.int64)
    preds = torch.softmax(torch.from_numpy(g.randn(nv * nc, C).astype(np.float32)) * 2, dim=1).numpy()
    preds[3] = preds[7]                                                       # equal rows: ties under "max"
    labels = video_labels[clip_ids // nc]
    splits = np.int64([4, 1, 7, 6])
    meter = ref.TestMeter(nv, nc, C, 4, multi_label=True, ensemble_method=mode)
    o = 0
    for n in splits:
        meter.update_stats(torch.from_numpy(preds[o:o + n]), torch.from_numpy(labels[o:o + n]), torch.from_numpy(clip_ids[o:o + n]))
        o += n
    meter.finalize_metrics()
    return {"preds": preds, "labels": labels, "clip_ids": clip_ids, "splits": splits,
            "video_preds": meter.video_preds.numpy().copy(), "video_labels": meter.video_labels.numpy().copy(),
            "clip_count": meter.clip_count.numpy().copy(), "map": np.float64(meter.stats["map"])}


def bce_records():
    g = np.random.RandomState(3)
    x = (g.randn(3, 7) * 4).astype(np.float32)
    x[0, :5] = np.float32([1e4, -1e4, 0.0, 30.0, -30.0])
    y = g.rand(3, 7).astype(np.float32)                                       # soft targets
    y[0, :5] = np.float32([1, 1, 0.5, 0, 0])
    y[1] = (y[1] > 0.5)                                                       # a multi-hot row
    p = g.rand(3, 7).astype(np.float32)
    p[0, :6] = np.float32([0, 0, 1, 1, 1e-8, 1e-8])
    yp = g.rand(3, 7).astype(np.float32)
    yp[0, :6] = np.float32([0, 1, 0, 1, 0, 1])
    out = {"bce.x": x, "bce.y": y, "bce.p": p, "bce.yp": yp}
    for name, fn, a, b in (("logit", torch.nn.functional.binary_cross_entropy_with_logits, x, y),
                           ("prob", torch.nn.functional.binary_cross_entropy, p, yp)):
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            for red in ("mean", "sum"):
                t = torch.from_numpy(a).to(dt).requires_grad_(True)
                loss = fn(t, torch.from_numpy(b).to(dt), reduction=red)
                loss.backward()
                out["bce.%s.%s.%s" % (name, tag, red)] = loss.detach().numpy()
                out["bce.%s.%s.grad_%s" % (name, tag, red)] = t.grad.numpy()
    return out


def main():
    from sklearn.metrics import average_precision_score
    ref = load_reference()
    out = {}
    for tag, (s, y) in ap_cases().items():
        out["ap.%s.scores" % tag], out["ap.%s.labels" % tag] = s, y
        out["ap.%s.map" % tag] = np.float64(ref.get_map(s, y))
        keep = ~np.all(y == 0, axis=0)
        if keep.any() and np.isfinite(s[:, keep]).all():
            out["ap.%s.aps" % tag] = np.atleast_1d(average_precision_score(y[:, keep], s[:, keep], average=None)).astype(np.float64)
        print(tag, s.shape, "map", out["ap.%s.map" % tag])
    for mode in ("max", "sum"):
        for k, v in test_meter_run(ref, mode).items():
            out["tm.%s.%s" % (mode, k)] = v
        print("TestMeter", mode, "map", out["tm.%s.map" % mode])
    out.update(bce_records())
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
