"""The AVA evaluation on the host (mirror of slowfast/utils/ava_eval_helper.py and of what its PascalDetectionEvaluator
computes: ava_evaluation/per_image_evaluation.py:261-352, object_detection_evaluation.py:640-830, metrics.py:21-125).  The
readers and the dict formats are the reference's; the arithmetic is one vectorised numpy pass over flat tables instead of
the evaluator's class tree and its call per (image, class):

  * a detection with not (y1 < y2 and x1 < x2) is dropped; excluded keys are dropped on both sides;
  * per (image, class) the detections are walked in input order -- not in score order -- and each takes the FIRST
    ground-truth row of its class with the largest float64 IoU if that IoU is >= 0.5 and the row is free (true positive),
    else it is a false positive; an image without ground truth of the class gives false positives, which count;
  * per class, with n ground-truth rows over all non-excluded ground-truth images, the rows are ordered by descending score
    and AP = sum_j (j / n - (j - 1) / n) max_{j' >= j} j' / (pos_j' + 1) over the true positives j = 1..m at 0-based ranks
    pos_j; NaN for n == 0, 0 without detections; mAP is the mean over the classes that are not NaN.

The one deviation: equal scores within a class are ordered by DESCENDING input position (for evaluate_ava: the row of the
concatenated update_stats calls), where the reference leaves them to numpy's unstable argsort."""
import csv
import logging
import time
from collections import defaultdict

import numpy as np

logger = logging.getLogger(__name__)

IOU_THRESHOLD = 0.5
MAP_KEY = "PascalBoxes_Precision/mAP@0.5IOU"
AP_KEY = "PascalBoxes_PerformanceByCategory/AP@0.5IOU/"


def make_image_key(video_id, timestamp):
    """'<video id>,<4-digit second>'."""
    return "%s,%04d" % (video_id, int(timestamp))


def read_csv(csv_file, class_whitelist=None, load_score=False):
    """AVA's CSV (video, second, x1, y1, x2, y2, class[, score]) -> (boxes, labels, scores): dicts from the image key to the
    lists of [y1, x1, y2, x2], of class ids and of scores (1.0 when the file has none).  Classes outside a non-empty
    whitelist are skipped."""
    boxes, labels, scores = defaultdict(list), defaultdict(list), defaultdict(list)
    with open(csv_file, "r") as f:
        for row in csv.reader(f):
            assert len(row) in [7, 8], "Wrong number of columns: %s" % (row,)
            action_id = int(row[6])
            if class_whitelist and action_id not in class_whitelist:
                continue
            key = make_image_key(row[0], row[1])
            x1, y1, x2, y2 = [float(n) for n in row[2:6]]
            boxes[key].append([y1, x1, y2, x2])
            labels[key].append(action_id)
            scores[key].append(float(row[7]) if load_score else 1.0)
    return boxes, labels, scores


def read_exclusions(exclusions_file):
    """The set of excluded image keys of a 'video,second' CSV; empty for no file."""
    excluded = set()
    if exclusions_file:
        with open(exclusions_file, "r") as f:
            for row in csv.reader(f):
                assert len(row) == 2, "Expected only 2 columns, got: %s" % (row,)
                excluded.add(make_image_key(row[0], row[1]))
    return excluded


def read_labelmap(labelmap_file):
    """The pbtxt label map -> ([{'id', 'name'}, ...] in file order, the set of ids)."""
    labelmap, class_ids, name = [], set(), ""
    with open(labelmap_file, "r") as f:
        for line in f:
            if line.startswith("  name:"):
                name = line.split('"')[1]
            elif line.startswith("  id:") or line.startswith("  label_id:"):
                class_id = int(line.strip().split(" ")[-1])
                labelmap.append({"id": class_id, "name": name})
                class_ids.add(class_id)
    return labelmap, class_ids


def get_ava_eval_data(scores, boxes, metadata, class_whitelist, verbose=False, video_idx_to_name=None):
    """Rows -> the evaluation's dicts: per row i and whitelisted class id c one entry under the key of
    (round(metadata[i][0]), round(metadata[i][1])) with the box of boxes[i, 1:5] as [y1, x1, y2, x2] and scores[i, c - 1]."""
    out_scores, out_labels, out_boxes = defaultdict(list), defaultdict(list), defaultdict(list)
    scores = np.asarray(scores)
    boxes = np.asarray(boxes)
    classes = [c for c in range(1, scores.shape[1] + 1) if c in class_whitelist] if scores.ndim == 2 else []
    for i in range(scores.shape[0]):
        key = video_idx_to_name[int(np.round(metadata[i][0]))] + "," + "%04d" % int(np.round(metadata[i][1]))
        b = boxes[i].tolist()
        box = [b[2], b[1], b[4], b[3]]
        row = scores[i].tolist()
        for c in classes:
            out_scores[key].append(row[c - 1])
            out_labels[key].append(c)
            out_boxes[key].append(box)
    return out_boxes, out_labels, out_scores


def write_results(detections, filename):
    """The official CSV: key, x1, y1, x2, y2 with three decimals, class, score with four."""
    boxes, labels, scores = detections
    with open(filename, "w") as f:
        for key in boxes.keys():
            for box, label, score in zip(boxes[key], labels[key], scores[key]):
                f.write("%s,%.03f,%.03f,%.03f,%.03f,%d,%.04f\n" % (key, box[1], box[0], box[3], box[2], label, score))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def pair_iou(det, gt):
    """IoU of paired rows [P,4] x [P,4] of [y1, x1, y2, x2] in float64, in the reference's order of operations."""
    area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    garea = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    ih = np.maximum(np.minimum(det[:, 2], gt[:, 2]) - np.maximum(det[:, 0], gt[:, 0]), 0.0)
    iw = np.maximum(np.minimum(det[:, 3], gt[:, 3]) - np.maximum(det[:, 1], gt[:, 1]), 0.0)
    inter = ih * iw
    return inter / (area + garea - inter)


def match_entries(num_classes, det_image, det_class, det_boxes, gt_image, gt_class, gt_boxes):
    """-> (valid bool [E], tp bool [E]).  Entries and ground-truth rows carry an integer image id and a 1-based class id; both
    are in input order.  The greedy walk is vectorised over the (image, class) groups: round r judges the r-th valid entry of
    every group at once."""
    det_image, det_class = np.asarray(det_image, np.int64), np.asarray(det_class, np.int64)
    det_boxes = np.asarray(det_boxes, np.float64).reshape(-1, 4)
    gt_image, gt_class = np.asarray(gt_image, np.int64), np.asarray(gt_class, np.int64)
    gt_boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    E = det_image.shape[0]
    valid = (det_boxes[:, 0] < det_boxes[:, 2]) & (det_boxes[:, 1] < det_boxes[:, 3])
    tp = np.zeros(E, dtype=bool)
    ent = np.flatnonzero(valid)
    if ent.size == 0 or gt_image.size == 0:
        return valid, tp
    stride = int(num_classes) + 1
    gkey = gt_image * stride + gt_class
    gorder = np.argsort(gkey, kind="stable")                    # file order survives within an (image, class)
    gkey = gkey[gorder]
    ekey = det_image[ent] * stride + det_class[ent]
    lo, hi = np.searchsorted(gkey, ekey, "left"), np.searchsorted(gkey, ekey, "right")
    cnt = hi - lo
    has = cnt > 0
    ent, ekey, lo, cnt = ent[has], ekey[has], lo[has], cnt[has]
    if ent.size == 0:
        return valid, tp
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    P = int(cnt.sum())
    within = np.arange(P) - np.repeat(start, cnt)
    iou = pair_iou(det_boxes[np.repeat(ent, cnt)], gt_boxes[gorder[np.repeat(lo, cnt) + within]])
    best = np.maximum.reduceat(iou, start)
    first = np.minimum.reduceat(np.where(iou == np.repeat(best, cnt), within, P), start)     # the first maximum
    cand = lo + first                                                                        # a row of the sorted ground truth
    eorder = np.argsort(ekey, kind="stable")
    sk = ekey[eorder]
    gstart = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    glen = np.diff(np.concatenate([gstart, [sk.size]]))
    rank = np.empty(ent.size, dtype=np.int64)
    rank[eorder] = np.arange(sk.size) - np.repeat(gstart, glen)
    taken = np.zeros(gkey.size, dtype=bool)
    hit = best >= IOU_THRESHOLD
    for r in range(int(rank.max()) + 1):
        sel = np.flatnonzero((rank == r) & hit)
        free = ~taken[cand[sel]]
        tp[ent[sel[free]]] = True
        taken[cand[sel[free]]] = True
    return valid, tp


def voc_ap(scores, tp, order, n_gt):
    """One class: float64 scores, the true-positive marks and the tie-break positions of its judged rows, n_gt ground-truth
    rows -> AP (NaN for n_gt == 0; ValueError for more true positives than ground truth, as in the reference)."""
    if n_gt == 0:
        return np.nan
    if int(np.sum(tp)) > n_gt:
        raise ValueError("Number of true positives must be smaller than num_gt.")
    if scores.size == 0 or not np.any(tp):
        return 0.0
    idx = np.lexsort((-np.asarray(order), -scores))             # descending score, then descending position
    pos = np.flatnonzero(tp[idx])
    j = np.arange(1, pos.size + 1, dtype=np.float64)
    env = np.maximum.accumulate((j / (pos + 1.0))[::-1])[::-1]
    return float(np.sum((j / n_gt - (j - 1.0) / n_gt) * env))


def evaluate_entries(num_classes, det_image, det_class, det_boxes, det_scores, det_order, gt_image, gt_class, gt_boxes):
    """The whole evaluation over flat tables (excluded images already dropped) -> dict(valid, tp: bool [E]; n_gt: int64
    [num_classes]; ap: float64 [num_classes]; map)."""
    det_class = np.asarray(det_class, np.int64)
    det_scores = np.asarray(det_scores, np.float64)
    det_order = np.asarray(det_order, np.int64)
    gt_class = np.asarray(gt_class, np.int64)
    if det_class.size and not np.all(np.isfinite(det_scores)):
        raise ValueError("evaluate_entries: a detection score is not finite")
    valid, tp = match_entries(num_classes, det_image, det_class, det_boxes, gt_image, gt_class, gt_boxes)
    n_gt = np.bincount(gt_class - 1, minlength=num_classes)[:num_classes].astype(np.int64)
    ap = np.full(num_classes, np.nan)
    by_class = np.argsort(det_class[valid], kind="stable")
    rows = np.flatnonzero(valid)[by_class]
    bounds = np.searchsorted(det_class[rows], np.arange(1, num_classes + 2))
    for c in range(num_classes):
        r = rows[bounds[c]:bounds[c + 1]]
        ap[c] = voc_ap(det_scores[r], tp[r], det_order[r], int(n_gt[c]))
    with np.errstate(invalid="ignore"):
        mean = float(np.nanmean(ap)) if np.any(~np.isnan(ap)) else float("nan")
    return {"valid": valid, "tp": tp, "n_gt": n_gt, "ap": ap, "map": mean}


def _flatten(table, excluded_keys, ids, with_scores):
    """(boxes, labels, scores) dicts -> flat arrays in dict order; `ids` maps image keys to integers and grows."""
    boxes, labels, scores = table
    image, cls, box, sc = [], [], [], []
    for key in boxes:
        if key in excluded_keys:
            continue
        n = len(boxes[key])
        image.append(np.full(n, ids.setdefault(key, len(ids)), dtype=np.int64))
        cls.append(np.asarray(labels[key], dtype=np.int64).reshape(n))
        box.append(np.asarray(boxes[key], dtype=np.float64).reshape(n, 4))
        if with_scores:
            sc.append(np.asarray(scores[key], dtype=np.float64).reshape(n))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)
    return cat(image, (0,), np.int64), cat(cls, (0,), np.int64), cat(box, (0, 4), np.float64), cat(sc, (0,), np.float64)


def _metrics(categories, ap, mean):
    out = {MAP_KEY: mean}
    names = {c["id"]: c["name"] for c in categories}
    for idx in range(ap.size):
        if idx + 1 in names:
            out[AP_KEY + names[idx + 1]] = ap[idx]
    return out


def _num_classes(categories):
    ids = [c["id"] for c in categories]
    if not ids or min(ids) < 1:
        raise ValueError("Classes should be 1-indexed.")
    return max(ids)


def run_evaluation(categories, groundtruth, detections, excluded_keys, verbose=True):
    """The reference's metric dict -- 'PascalBoxes_Precision/mAP@0.5IOU' and one
    'PascalBoxes_PerformanceByCategory/AP@0.5IOU/<name>' per category -- from the (boxes, labels, scores) dicts.  Classes
    are the ids 1..max id of `categories`; a detection of a larger class id is refused.  The tie-break position of an entry
    is its place in the dicts' order."""
    C = _num_classes(categories)
    ids = {}
    gi, gc, gb, _ = _flatten(groundtruth, excluded_keys, ids, False)
    di, dc, db, ds = _flatten(detections, excluded_keys, ids, True)
    for what, cls in (("ground-truth", gc), ("detection", dc)):
        if cls.size and (cls.min() < 1 or cls.max() > C):
            raise ValueError("run_evaluation: a %s class id lies outside 1..%d" % (what, C))
    res = evaluate_entries(C, di, dc, db, ds, np.arange(di.size), gi, gc, gb)
    metrics = _metrics(categories, res["ap"], res["map"])
    if verbose:
        logger.info("AVA evaluation: %s", metrics)
    return metrics


def evaluate_arrays(preds, original_boxes, metadata, excluded_keys, class_whitelist, categories, groundtruth,
                    video_idx_to_name):
    """evaluate_ava's arithmetic without the dicts: one entry per (row, whitelisted class) in row-major order, the row as
    tie-break position -> the dict of evaluate_entries plus `rows`, `classes` (per entry) and `kept` (bool per row: its image
    is not excluded)."""
    preds = np.asarray(preds, dtype=np.float32)
    original_boxes = np.asarray(original_boxes, dtype=np.float32).reshape(-1, 5)
    metadata = np.asarray(metadata, dtype=np.float64).reshape(preds.shape[0], -1)
    C = _num_classes(categories)
    if preds.ndim != 2 or preds.shape[1] < C or original_boxes.shape[0] != preds.shape[0]:
        raise ValueError("evaluate_ava takes preds [K,>=%d], original_boxes [K,5] and metadata [K,2]; got %s, %s, %s" % (
            C, preds.shape, original_boxes.shape, metadata.shape))
    ids = {}
    gi, gc, gb, _ = _flatten(groundtruth, excluded_keys, ids, False)
    if gc.size and (gc.min() < 1 or gc.max() > C):
        raise ValueError("evaluate_ava: a ground-truth class id lies outside 1..%d" % C)
    K = preds.shape[0]
    vid, sec = np.round(metadata[:, 0]).astype(np.int64), np.round(metadata[:, 1]).astype(np.int64)
    image = np.empty(K, dtype=np.int64)
    kept = np.ones(K, dtype=bool)
    cache = {}
    for i, pair in enumerate(zip(vid.tolist(), sec.tolist())):
        if pair not in cache:
            key = video_idx_to_name[pair[0]] + "," + "%04d" % pair[1]
            cache[pair] = -1 if key in excluded_keys else ids.setdefault(key, len(ids))
        image[i] = cache[pair]
        kept[i] = cache[pair] >= 0
    classes = np.array([c for c in range(1, C + 1) if c in class_whitelist], dtype=np.int64)
    rows = np.repeat(np.flatnonzero(kept), classes.size)
    cls = np.tile(classes, int(kept.sum()))
    yxyx = original_boxes[:, [2, 1, 4, 3]].astype(np.float64)
    res = evaluate_entries(C, image[rows], cls, yxyx[rows], preds[rows, cls - 1].astype(np.float64), rows, gi, gc, gb)
    res.update(rows=rows, classes=cls, kept=kept)
    return res


def evaluate_ava(preds, original_boxes, metadata, excluded_keys, class_whitelist, categories, groundtruth=None,
                 video_idx_to_name=None, name="latest", write_csv=False):
    """mAP@0.5IOU of the rows of an epoch.  preds [K,C] scores, original_boxes [K,5] (batch index, x1, y1, x2, y2), metadata
    [K,2] (video index, second).  The reference also writes detections_<name>.csv and groundtruth_<name>.csv on every call;
    here only with write_csv=True."""
    start = time.time()
    preds = preds.detach().float().cpu().numpy() if hasattr(preds, "detach") else preds
    original_boxes = original_boxes.detach().float().cpu().numpy() if hasattr(original_boxes, "detach") else original_boxes
    metadata = metadata.detach().cpu().tolist() if hasattr(metadata, "detach") else metadata
    if write_csv:
        write_results(get_ava_eval_data(preds, original_boxes, metadata, class_whitelist, video_idx_to_name=video_idx_to_name),
                      "detections_%s.csv" % name)
        write_results(groundtruth, "groundtruth_%s.csv" % name)
    res = evaluate_arrays(preds, original_boxes, metadata, excluded_keys, class_whitelist, categories, groundtruth,
                          video_idx_to_name)
    logger.info("AVA eval done in %f seconds." % (time.time() - start))
    return res["map"]
