"""TEST INFRASTRUCTURE shared by test_ava_eval_ref_cpu.py and test_gpu_ava_eval.py: the cases of tests/golden/ava_eval.npz,
their annotation files written out again, and the comparison with what the reference recorded."""
import os

import numpy as np

from conftest import GOLDEN

U = 2.0 ** -52


def load():
    z = np.load(os.path.join(GOLDEN, "ava_eval.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def case(z, tag):
    return {k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + ".")}


def write_annotations(c, root):
    """The annotation directory of a case: ground truth, exclusions, label map and a frame list that numbers the videos."""
    root = str(root)
    os.makedirs(root, exist_ok=True)
    for name, key in (("gt.csv", "gt_csv"), ("excl.csv", "excl_csv"), ("labelmap.pbtxt", "labelmap")):
        with open(os.path.join(root, name), "w") as f:
            f.write(str(c[key]))
    for name in ("val.csv", "train.csv"):
        with open(os.path.join(root, name), "w") as f:
            f.write("original_video_id video_id frame_id path labels\n")
            for i, n in enumerate(c["names"]):
                for fr in range(2):
                    f.write('%s %d %d %s/%s_%06d.jpg ""\n' % (n, i, fr, n, n, fr))
    return root


def make_cfg(root, full_on_val=False):
    from focus_amd.slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.AVA.ANNOTATION_DIR = cfg.AVA.FRAME_LIST_DIR = str(root)
    cfg.AVA.FRAME_DIR = "frames"
    cfg.AVA.GROUNDTRUTH_FILE, cfg.AVA.EXCLUSION_FILE, cfg.AVA.LABEL_MAP_FILE = "gt.csv", "excl.csv", "labelmap.pbtxt"
    cfg.AVA.FULL_TEST_ON_VAL = full_on_val
    return cfg


def unflatten(c, prefix, with_scores):
    """The flattened dicts of the fixture -> (boxes, labels, scores) dicts in their order."""
    boxes, labels, scores = {}, {}, {}
    o = 0
    for k, n in zip(c[prefix + ".keys"].tolist(), c[prefix + ".counts"].tolist()):
        boxes[k] = c[prefix + ".boxes"][o:o + n].astype(np.float64).tolist()
        labels[k] = c[prefix + ".labels"][o:o + n].astype(np.int64).tolist()
        scores[k] = c[prefix + ".scores"][o:o + n].astype(np.float64).tolist() if with_scores else [1.0] * n
        o += n
    return boxes, labels, scores


def row_keys(c):
    return ["%s,%04d" % (c["names"][int(np.round(m[0]))], int(np.round(m[1]))) for m in c["metadata"]]


def check_bytes(c, by, what=""):
    """The bytes [K,C] (0 / 1 false positive / 2 true positive) against the evaluator's tp_fp_labels_per_class: per class the
    same rows -- found by their scores -- in the evaluator's order (images by first arrival, rows in arrival order)."""
    keys = row_keys(c)
    arrival = {}
    for k in keys:
        arrival.setdefault(k, len(arrival))
    order = sorted(range(len(keys)), key=lambda r: (arrival[keys[r]], r))
    off = c["cls.offsets"]
    num = off.size - 1
    assert not by[:, num:].any(), what + ": a column past the label map's largest id was judged"
    for cl in range(num):
        rows = [r for r in order if by[r, cl] != 0]
        assert np.array_equal(c["preds"][rows, cl].astype(np.float64), c["cls.scores"][off[cl]:off[cl + 1]]), (what, cl)
        assert np.array_equal(by[rows, cl] == 2, c["cls.tp"][off[cl]:off[cl + 1]]), (what, cl)


def check_ap(c, ap, mean, what="", exact_from=None):
    """|dAP_c| <= (m_c - 1) 2^-52: both sides add the same m_c non-negative terms, whose total is at most 1, in different
    orders, each with an error of at most (m_c - 1) 2^-53.  The mean over the K kept classes: the inputs differ by at most
    sum_c (m_c - 1) 2^-52 in total; each side adds K values <= 1 with at most (K - 1) roundings of partial sums <= K, an
    error of at most (K - 1) K 2^-53 per side; the division by K turns that into (K - 1) 2^-52 for the two sides together,
    and rounds the quotient (<= 1) once per side: 2^-53 each.
        |d mean| <= (sum_c (m_c - 1) / K + (K - 1) + 1) 2^-52."""
    ref = c["ap"]
    num = ref.size
    ap = np.asarray(ap, dtype=np.float64)
    assert np.array_equal(np.isnan(ap[:num]), np.isnan(ref)), what + ": NaN pattern"
    assert np.all(np.isnan(ap[num:])), what
    off = c["cls.offsets"]
    m = np.array([int(c["cls.tp"][off[k]:off[k + 1]].sum()) for k in range(num)])
    kept = ~np.isnan(ref)
    bound = np.maximum(m - 1, 0) * U
    diff = np.abs(ap[:num][kept] - ref[kept])
    assert np.all(diff <= bound[kept]), (what, diff.max(), bound[kept].max())
    K = int(kept.sum())
    mean_bound = (np.maximum(m[kept] - 1, 0).sum() / K + (K - 1) + 1) * U
    print("%s: max |dAP| %.3g (bound up to %.3g), |d mean| %.3g (bound %.3g)" % (
        what, diff.max(), bound[kept].max(), abs(mean - float(c["map"])), mean_bound))
    assert abs(mean - float(c["map"])) <= mean_bound, (what, mean, float(c["map"]))
    if exact_from is not None:
        assert np.array_equal(ap, exact_from, equal_nan=True), what + ": not bit-equal to the twin"
    return bound, mean_bound
