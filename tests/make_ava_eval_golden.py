"""TEST INFRASTRUCTURE: writes tests/golden/ava_eval.npz from the reference's own slowfast/utils/ava_eval_helper.py and
slowfast/utils/ava_evaluation/, loaded from their files (slowfast.utils.distributed and slowfast.utils.env are stubs; the
numpy aliases np.bool, np.float and np.NAN, which numpy 2 removed, are set at run time).  Runs only where the reference tree is
present:
    python tests/make_ava_eval_golden.py
The fixture is data only.  Per case (`edge`: the hand-made situations listed in cases(); `random`: about 300 box rows x 80
classes, 60 of them whitelisted):
  <case>.{preds, boxes, metadata, splits, names}   the rows an AVAMeter receives, the batch sizes, video_idx_to_name
  <case>.{gt_csv, excl_csv, labelmap}               the annotation files as strings
  <case>.det.{keys, counts, boxes, labels, scores}  get_ava_eval_data's three dicts, flattened in dict order
  <case>.cls.{offsets, scores, tp}                  the evaluator's scores_per_class / tp_fp_labels_per_class, concatenated
  <case>.{n_gt, ap, map}                            num_gt_instances_per_class, the per-class AP, the mAP
  <case>.gt.{keys, counts, boxes, labels}, <case>.{excluded, label_ids, label_names, mini_keys}   what read_csv,
      read_exclusions, read_labelmap and get_ava_mini_groundtruth returned for the strings
  dicts.*   a run_evaluation call on hand-made dicts in which a class has ground truth and no detection entry at all.
The maker asserts that the scores are distinct within every class: the order of equal scores is an artefact of the
reference's unstable sort."""
import importlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "ava_eval.npz")


def load_reference():
    from oracle._ref_loader import REF
    np.bool, np.float, np.NAN = bool, float, np.nan             # numpy 2 removed the aliases the TF port uses
    for name in ("slowfast", "slowfast.utils"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    du = types.ModuleType("slowfast.utils.distributed")
    du.is_master_proc = lambda *a, **k: False
    env = types.ModuleType("slowfast.utils.env")
    env.pathmgr = types.SimpleNamespace(open=open)
    sys.modules["slowfast.utils.distributed"], sys.modules["slowfast.utils.env"] = du, env
    sys.modules["slowfast.utils"].distributed, sys.modules["slowfast.utils"].env = du, env
    pkg = types.ModuleType("slowfast.utils.ava_evaluation")
    pkg.__path__ = [os.path.join(REF, "slowfast", "utils", "ava_evaluation")]
    sys.modules["slowfast.utils.ava_evaluation"] = pkg
    sys.modules["slowfast.utils"].ava_evaluation = pkg
    ode = importlib.import_module("slowfast.utils.ava_evaluation.object_detection_evaluation")
    importlib.import_module("slowfast.utils.ava_evaluation.standard_fields")
    spec = importlib.util.spec_from_file_location("slowfast.utils.ava_eval_helper",
                                                  os.path.join(REF, "slowfast", "utils", "ava_eval_helper.py"))
    helper = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helper)
    return helper, ode


def mini_groundtruth(full):
    """The reference's get_ava_mini_groundtruth lives in meters.py, which needs fvcore and scikit-learn; its rule is one
    line (keys whose second is a multiple of 4) and only the resulting key list is recorded."""
    return [k for k in full[0].keys() if int(k.split(",")[1]) % 4 == 0]


def labelmap_text(ids):
    return "".join('item {\n  name: "action %d"\n  id: %d\n}\n' % (i, i) if i % 2 else
                   'label {\n  name: "action %d"\n  label_id: %d\n  label_type: PERSON_MOVEMENT\n}\n' % (i, i) for i in ids)


def distinct_scores(g, K, C):
    """fp32 scores in (0, 1), distinct within every column."""
    s = np.stack([(g.permutation(K) + g.uniform(0.2, 0.8, K)) / K for _ in range(C)], axis=1).astype(np.float32)
    for c in range(C):
        assert np.unique(s[:, c]).size == K
    return s


def iou64(d, t):
    ih = max(min(d[3], t[3]) - max(d[1], t[1]), 0.0)
    iw = max(min(d[2], t[2]) - max(d[0], t[0]), 0.0)
    inter = ih * iw
    return inter / ((d[3] - d[1]) * (d[2] - d[0]) + (t[3] - t[1]) * (t[2] - t[0]) - inter)


def iou32(d, t):
    f = np.float32
    d, t = [f(v) for v in d], [f(v) for v in t]
    ih = max(min(d[3], t[3]) - max(d[1], t[1]), f(0))
    iw = max(min(d[2], t[2]) - max(d[0], t[0]), f(0))
    inter = f(ih * iw)
    return f(inter / f(f(f(f(d[3] - d[1]) * f(d[2] - d[0])) + f(f(t[3] - t[1]) * f(t[2] - t[0]))) - inter))


def threshold_pairs(g, want):
    """(detection, ground truth) pairs whose IoU is about one half -- the detection is twice as tall -- and for which float64
    and fp32 arithmetic fall on different sides of 0.5.  Ground-truth coordinates have three decimals; detections are fp32."""
    out = {True: [], False: []}
    while min(len(v) for v in out.values()) < want:
        x1, y1 = round(g.uniform(0.05, 0.3), 3), round(g.uniform(0.05, 0.3), 3)
        w, h = round(g.uniform(0.1, 0.3), 3), round(g.uniform(0.1, 0.3), 3)
        gt = [x1, y1, round(x1 + w, 3), round(y1 + h, 3)]
        det = [float(np.float32(v)) for v in (x1, y1, round(x1 + w, 3), round(y1 + 2 * h, 3))]
        a, b = iou64(det, gt) >= 0.5, iou32(det, gt) >= np.float32(0.5)
        if a != b:
            out[bool(a)].append((det, gt))
    return out[True][:want] + out[False][:want]


def edge_case():
    g = np.random.RandomState(5)
    names = ["vidA", "vidB", "vidC"]
    whitelist = [1, 2, 3, 4, 5, 7]                              # 6 is not in the label map; column 8 lies past its largest id
    gt, det = [], []                                            # (video, sec, box, class) / (video idx, sec, box)
    # vidA,0904: the IoU of exactly 0.5; two detections on one row; two equal rows in one class; an invalid box
    gt += [("vidA", 904, (0, 0, 1, 0.5), 1), ("vidA", 904, (0.1, 0.1, 0.5, 0.5), 2), ("vidA", 904, (0.1, 0.1, 0.5, 0.5), 3),
           ("vidA", 904, (0.1, 0.1, 0.5, 0.5), 3), ("vidA", 904, (0.6, 0.6, 0.9, 0.9), 4)]
    det += [(0, 904, (0, 0, 1, 1)), (0, 904, (0.1, 0.1, 0.5, 0.5)), (0, 904, (0.1, 0.1, 0.5, 0.52)), (0, 904, (0.3, 0.3, 0.3, 0.9))]
    gt += [("vidA", 905, (0.2, 0.2, 0.7, 0.7), 1), ("vidA", 905, (0.2, 0.2, 0.7, 0.7), 5)]      # ground truth, no detection
    det += [(1, 10, (0.2, 0.2, 0.6, 0.6)), (1, 10, (0.5, 0.1, 0.9, 0.8))]                        # detections, no ground truth
    gt += [("vidB", 12, (0.1, 0.1, 0.4, 0.4), 1), ("vidB", 12, (0.1, 0.1, 0.4, 0.4), 2)]        # excluded on both sides
    det += [(1, 12, (0.1, 0.1, 0.4, 0.4))]
    # vidC: decimals that fp32 cannot hold, at the threshold, one pair per image; vidC,0008 gets a second row and arrives in
    # two batches (see the order below)
    for sec, (d, t) in zip((8, 16, 21, 22), threshold_pairs(g, 2)):
        gt.append(("vidC", sec, tuple(t), 5))
        det.append((2, sec, tuple(d)))
    gt.append(("vidC", 8, (0.123, 0.457, 0.789, 0.913), 2))
    det.append((2, 8, (0.123, 0.457, 0.789, 0.913)))
    # vidA,0906: a detection that ties at 0.5 between two different rows of class 4 takes the first; the next one wants it too
    gt += [("vidA", 906, (0, 0, 1, 0.5), 4), ("vidA", 906, (0, 0.5, 1, 1), 4)]
    det += [(0, 906, (0, 0, 1, 1)), (0, 906, (0, 0, 1, 0.55))]
    order = [0, 1, 7, 4, 2, 3, 8, 5, 6, 9, 10, 11, 12, 13]              # vidC,0008 (rows 7 and 11) lies in the first and the last batch
    det = [det[i] for i in order]
    K, C = len(det), 8
    preds = distinct_scores(g, K, C)
    preds[order.index(2), 1] = np.float32(0.99)                 # the later detection of the shared row scores higher
    preds[order.index(1), 1] = np.float32(0.5)
    boxes = np.float32([[i % 3] + list(d[2]) for i, d in enumerate(det)])
    metadata = np.float64([[d[0] + 0.2 * (i % 2) - 0.1, d[1] - 0.3 * (i % 2)] for i, d in enumerate(det)])   # rounded by the reader
    gt_csv = "".join("%s,%04d,%s,%d,%d\n" % (v, s, ",".join("%.3f" % x for x in b), c, i) for i, (v, s, b, c) in enumerate(gt))
    gt_csv += "vidA,0904,0.100,0.100,0.500,0.500,6,77\n"        # a class outside the whitelist: dropped by the reader
    return dict(preds=preds, boxes=boxes, metadata=metadata, splits=np.int64([3, 1, 5, 5]), names=names, gt_csv=gt_csv,
                excl_csv="vidB,0012\nvidZ,0001\n", labelmap=labelmap_text(whitelist))


def random_case():
    g = np.random.RandomState(9)
    C = 80
    whitelist = sorted(g.permutation(np.arange(1, C + 1))[:60].tolist())
    names = ["v%02d" % i for i in range(10)]
    keys = [(v, s) for v in range(10) for s in range(900, 910)]
    freq = 1.0 / (1.0 + g.permutation(C))                       # a few frequent classes, many rare ones, as in AVA
    freq /= freq.sum()
    gt_lines, det, excl = [], [], []
    for v, s in keys:
        kind = g.rand()
        persons = [np.round(np.r_[lo, lo + g.uniform(0.15, 0.5, 2)], 3) for lo in g.uniform(0.0, 0.45, (g.randint(1, 5), 2))]
        if kind < 0.06:
            excl.append((v, s))
        if kind < 0.85 or kind >= 0.95:                         # 10 %: no ground truth for the image
            for pid, b in enumerate(persons):
                labels = g.choice(np.arange(1, C + 1), size=g.randint(1, 4), replace=False, p=freq)
                if g.rand() < 0.15:
                    labels = np.r_[labels, labels[:1]]          # the same (box, class) twice: equal rows
                for c in labels:
                    gt_lines.append("%s,%04d,%.3f,%.3f,%.3f,%.3f,%d,%d\n" % (names[v], s, b[0], b[1], b[2], b[3], c, pid))
        if kind >= 0.12:                                        # a few images have ground truth and no detection
            for _ in range(g.randint(1, 7)):
                b = persons[g.randint(len(persons))] + g.normal(0, g.choice([0.01, 0.05, 0.12]), 4)
                if g.rand() < 0.04:
                    b[2] = b[0]                                 # invalid
                det.append((v, s, b))
    g.shuffle(det)
    K = len(det)
    preds = distinct_scores(g, K, C)
    boxes = np.float32([[0] + list(b) for _, _, b in det])
    metadata = np.float64([[v, s] for v, s, _ in det])
    splits, left = [], K
    while left:
        n = min(left, int(g.randint(1, 64)))
        splits.append(n)
        left -= n
    return dict(preds=preds, boxes=boxes, metadata=metadata, splits=np.int64(splits), names=names, gt_csv="".join(gt_lines),
                excl_csv="".join("%s,%04d\n" % (names[v], s) for v, s in excl), labelmap=labelmap_text(whitelist))


def cases():
    return {"edge": edge_case(), "random": random_case()}


def flatten(table, with_scores, box_dtype):
    boxes, labels, scores = table
    keys = list(boxes.keys())
    out = {"keys": np.array(keys), "counts": np.int64([len(boxes[k]) for k in keys]),
           "boxes": np.array([b for k in keys for b in boxes[k]], dtype=np.float64).reshape(-1, 4),
           "labels": np.array([l for k in keys for l in labels[k]], dtype=np.int16)}
    assert np.array_equal(out["boxes"].astype(box_dtype).astype(np.float64), out["boxes"])
    out["boxes"] = out["boxes"].astype(box_dtype)
    if with_scores:
        s = np.array([x for k in keys for x in scores[k]], dtype=np.float64)
        assert np.array_equal(s.astype(box_dtype).astype(np.float64), s)
        out["scores"] = s.astype(box_dtype)
    return out


def evaluate(helper, ode, categories, groundtruth, detections, excluded):
    """run_evaluation of the reference, with the evaluator it builds caught on the way."""
    caught = []
    real = ode.PascalDetectionEvaluator.__init__

    def catching(self, *a, **k):
        real(self, *a, **k)
        caught.append(self)
    ode.PascalDetectionEvaluator.__init__ = catching
    try:
        metrics = helper.run_evaluation(categories, groundtruth, detections, excluded)
    finally:
        ode.PascalDetectionEvaluator.__init__ = real
    ev = caught[0]._evaluation
    C = ev.num_class
    sc = [np.concatenate(x) if x else np.zeros(0) for x in ev.scores_per_class]
    tp = [np.concatenate(x) if x else np.zeros(0, bool) for x in ev.tp_fp_labels_per_class]
    for c in range(C):
        assert np.unique(sc[c]).size == sc[c].size, "scores of class %d are not distinct" % (c + 1)
    out = {"cls.offsets": np.int64(np.r_[0, np.cumsum([x.size for x in sc])]),
           "cls.scores": np.concatenate(sc).astype(np.float64), "cls.tp": np.concatenate(tp).astype(bool),
           "n_gt": np.int64(ev.num_gt_instances_per_class), "ap": np.float64(ev.average_precision_per_class),
           "map": np.float64(metrics["PascalBoxes_Precision/mAP@0.5IOU"])}
    names = {c["id"]: c["name"] for c in categories}
    for c in range(C):
        if c + 1 in names:
            v = metrics["PascalBoxes_PerformanceByCategory/AP@0.5IOU/" + names[c + 1]]
            assert (np.isnan(v) and np.isnan(out["ap"][c])) or v == out["ap"][c]
    return out


def record(helper, ode, tag, case):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for k in ("gt_csv", "excl_csv", "labelmap"):
            paths[k] = os.path.join(d, k)
            with open(paths[k], "w") as f:
                f.write(case[k])
        categories, whitelist = helper.read_labelmap(paths["labelmap"])
        excluded = helper.read_exclusions(paths["excl_csv"])
        groundtruth = helper.read_csv(paths["gt_csv"], whitelist)
    detections = helper.get_ava_eval_data(case["preds"], case["boxes"], case["metadata"].tolist(), whitelist,
                                          video_idx_to_name=case["names"])
    for k in ("preds", "boxes", "metadata", "splits"):
        out[k] = case[k]
    out["names"] = np.array(case["names"])
    for k in ("gt_csv", "excl_csv", "labelmap"):
        out[k] = np.array(case[k])
    for k, v in flatten(detections, True, np.float32).items():
        out["det." + k] = v
    for k, v in flatten(groundtruth, False, np.float64).items():
        out["gt." + k] = v
    out["excluded"] = np.array(sorted(excluded))
    out["label_ids"] = np.int64([c["id"] for c in categories])
    out["label_names"] = np.array([c["name"] for c in categories])
    out["mini_keys"] = np.array(mini_groundtruth(groundtruth))
    out.update(evaluate(helper, ode, categories, groundtruth, detections, excluded))
    print(tag, "rows", case["preds"].shape, "entries", out["det.labels"].size, "gt rows", out["gt.labels"].size, "n_gt>0",
          int((out["n_gt"] > 0).sum()), "TP", int(out["cls.tp"].sum()), "mAP", out["map"])
    return {"%s.%s" % (tag, k): v for k, v in out.items()}


def dict_case(helper, ode):
    """Hand-made dicts: class 2 has ground truth and no detection entry (AP 0); class 3 no ground truth (NaN)."""
    categories = [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}, {"id": 3, "name": "c"}]
    gt = ({"k,0001": [[0.1, 0.1, 0.5, 0.5], [0.1, 0.1, 0.5, 0.5]], "k,0002": [[0.2, 0.2, 0.6, 0.6]]},
          {"k,0001": [1, 2], "k,0002": [1]}, {"k,0001": [1.0, 1.0], "k,0002": [1.0]})
    det = ({"k,0001": [[0.1, 0.1, 0.5, 0.5], [0.1, 0.1, 0.5, 0.5]], "k,0002": [[0.0, 0.0, 0.1, 0.1], [0.2, 0.2, 0.6, 0.6]]},
           {"k,0001": [1, 3], "k,0002": [1, 1]}, {"k,0001": [0.3, 0.9], "k,0002": [0.8, 0.6]})
    res = evaluate(helper, ode, categories, gt, det, set())
    assert res["ap"][1] == 0.0 and np.isnan(res["ap"][2])
    out = {"dicts.ap": res["ap"], "dicts.map": res["map"], "dicts.n_gt": res["n_gt"]}
    for name, table in (("gt", gt), ("det", det)):
        for k, v in flatten(table, True, np.float64).items():
            out["dicts.%s.%s" % (name, k)] = v
    print("dicts ap", res["ap"], "mAP", res["map"])
    return out


def main():
    helper, ode = load_reference()
    out = {}
    for tag, case in cases().items():
        out.update(record(helper, ode, tag, case))
    out.update(dict_case(helper, ode))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
