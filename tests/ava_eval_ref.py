"""TEST INFRASTRUCTURE: the plain-loop float64 twin of csrc/ava_eval.hip (include/focus_amd.h, "The AVA evaluation").

match(...)   focus_ava_match over the same tables -> (bytes uint8 [K,C], counts int64 [2,C], flag)
voc_ap(...)  focus_voc_ap -> (ap float64 [C], summary float64 [2], flag), the double sums in the kernel's stated order
tables(...)  rows as an AVAMeter receives them + annotation dicts -> the tables both take (what DeviceAVAMeter builds)
Every `mutant` is one deliberate mistake; tests/test_ava_eval_ref_cpu.py shows that each leaves the recorded output."""
import numpy as np

GT_CAP = 64
MATCH_GT_OVERFLOW, MATCH_BAD_INDEX = 1, 2
VOC_BAD_SCORE, VOC_TP_ABOVE_GT, VOC_GT_ABOVE_TOTAL = 1, 2, 4
MUTANTS = ("score_order", "strict_threshold", "last_maximum", "no_envelope", "fp32_iou", "keep_invalid", "detected_images_only")


def _iou(d, t, f):
    """d, t: (x1, y1, x2, y2); f: the number type of every operation."""
    d, t = [f(v) for v in d], [f(v) for v in t]
    area = f(f(d[3] - d[1]) * f(d[2] - d[0]))
    garea = f(f(t[3] - t[1]) * f(t[2] - t[0]))
    ih = max(f(min(d[3], t[3]) - max(d[1], t[1])), f(0))
    iw = max(f(min(d[2], t[2]) - max(d[0], t[0])), f(0))
    inter = f(ih * iw)
    return f(inter / f(f(area + garea) - inter))


def match(boxes, C, grp_off, det_rows, grp_image, gt_off, gt_class, gt_boxes, whitelist, scores=None, mutant=None):
    K = boxes.shape[0]
    out = np.zeros((K, C), dtype=np.uint8)
    counts = np.zeros((2, C), dtype=np.int64)
    flag = 0
    f = np.float32 if mutant == "fp32_iou" else np.float64
    for g in range(len(grp_image)):
        im = int(grp_image[g])
        t0, t1 = (int(gt_off[im]), int(gt_off[im + 1])) if im >= 0 else (0, 0)
        rows = [int(r) for r in det_rows[int(grp_off[g]):int(grp_off[g + 1])]]
        for c in range(C):
            if not whitelist[c]:
                continue
            gts = [t for t in range(t0, t1) if gt_class[t] == c + 1]
            if len(gts) > GT_CAP:
                flag |= MATCH_GT_OVERFLOW
                continue
            walk = rows
            if mutant == "score_order":
                walk = sorted(rows, key=lambda r: -float(scores[r, c]))
            taken = set()
            for r in walk:
                x1, y1, x2, y2 = [float(v) for v in boxes[r]]
                if not (y1 < y2 and x1 < x2) and mutant != "keep_invalid":
                    continue
                best, best_t = -1.0, -1
                for k, t in enumerate(gts):
                    with np.errstate(invalid="ignore", divide="ignore"):
                        v = float(_iou(boxes[r], gt_boxes[t], f))
                    if v > best or (mutant == "last_maximum" and v == best):
                        best, best_t = v, k
                hit = best > 0.5 if mutant == "strict_threshold" else best >= 0.5
                tp = best_t >= 0 and hit and best_t not in taken
                if tp:
                    taken.add(best_t)
                out[r, c] = 2 if tp else 1
                counts[0, c] += 1
                counts[1, c] += int(tp)
    return out, counts, flag


def voc_ap(scores, bytes_, n_gt, total_gt=None, mutant=None):
    """scores [N,C] (fp32 values), bytes_ uint8 [N,C], n_gt int64 [C]."""
    N, C = bytes_.shape
    total_gt = int(np.sum(np.maximum(n_gt, 0))) if total_gt is None else int(total_gt)
    ap = np.full(C, np.nan)
    flag, at = 0, 0
    for c in range(C):
        n = max(int(n_gt[c]), 0)
        room = n <= total_gt - at
        if room:
            at += n
        else:
            flag |= VOC_GT_ABOVE_TOTAL
        rows = [i for i in range(N) if bytes_[i, c] != 0]
        if any(not np.isfinite(scores[i, c]) for i in rows):
            flag |= VOC_BAD_SCORE
        rows.sort(key=lambda i: (-float(scores[i, c]), -i))      # descending score, equal scores by descending row
        pos = [p for p, i in enumerate(rows) if bytes_[i, c] == 2]
        m = len(pos)
        if m > n > 0:
            flag |= VOC_TP_ABOVE_GT
        if n == 0 or m > n or not room:
            continue
        prec = [np.float64(j + 1) / np.float64(pos[j] + 1) for j in range(m)]
        L = -(-m // 256)
        parts = [np.float64(0.0)] * 256
        for k in range(256):
            a, b = min(k * L, m), min(k * L + L, m)
            env = max(prec[b:], default=np.float64(0.0))
            acc = np.float64(0.0)
            for j in range(b - 1, a - 1, -1):
                env = max(env, prec[j])
                step = np.float64(j + 1) / np.float64(n) - np.float64(j) / np.float64(n)
                acc = acc + step * (prec[j] if mutant == "no_envelope" else env)
            parts[k] = acc
        h = 128
        while h:
            for s in range(h):
                parts[s] = parts[s] + parts[s + h]
            h //= 2
        ap[c] = parts[0]
    total, kept = np.float64(0.0), 0
    for c in range(C):
        if n_gt[c] > 0 and not np.isnan(ap[c]):
            total = total + ap[c]
            kept += 1
    return ap, np.float64([total / kept if kept else np.nan, kept]), flag


def tables(metadata, names, groundtruth, excluded, whitelist_ids, C, mutant=None):
    """-> dict(grp_off, det_rows, grp_image, gt_off, gt_class, gt_boxes, whitelist, n_gt, keys): the detection rows grouped by
    image key in first-arrival order, the ground truth (the reader's dicts, boxes [y1, x1, y2, x2]) by image in dict order
    with boxes as (x1, y1, x2, y2), excluded keys dropped on both sides."""
    gt_keys = [k for k in groundtruth[0] if k not in excluded]
    image_of = {k: i for i, k in enumerate(gt_keys)}
    gt_off, gt_class, gt_boxes = [0], [], []
    for k in gt_keys:
        for b, l in zip(groundtruth[0][k], groundtruth[1][k]):
            gt_class.append(l)
            gt_boxes.append([b[1], b[0], b[3], b[2]])
        gt_off.append(len(gt_class))
    groups, keys = {}, []
    for i in range(len(metadata)):
        key = "%s,%04d" % (names[int(np.round(metadata[i][0]))], int(np.round(metadata[i][1])))
        keys.append(key)
        if key not in excluded:
            groups.setdefault(key, []).append(i)
    det_rows = np.full(len(metadata), -1, dtype=np.int64)
    flat = [r for rows in groups.values() for r in rows]
    det_rows[:len(flat)] = flat
    gt_class = np.asarray(gt_class, dtype=np.int32).reshape(-1)
    n_gt = np.zeros(C, dtype=np.int64)
    seen = set(groups)
    for k, a, b in zip(gt_keys, gt_off[:-1], gt_off[1:]):
        if mutant == "detected_images_only" and k not in seen:
            continue
        for l in gt_class[a:b]:
            n_gt[l - 1] += 1
    whitelist = np.zeros(C, dtype=np.uint8)
    for c in whitelist_ids:
        if 1 <= c <= C:
            whitelist[c - 1] = 1
    return dict(grp_off=np.int64(np.r_[0, np.cumsum([len(v) for v in groups.values()])]), det_rows=det_rows,
                grp_image=np.int64([image_of.get(k, -1) for k in groups]), gt_off=np.int64(gt_off), gt_class=gt_class,
                gt_boxes=np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), whitelist=whitelist, n_gt=n_gt, keys=keys)


def evaluate(preds, boxes, metadata, names, groundtruth, excluded, whitelist_ids, num_classes, mutant=None):
    """The whole route on the twin: -> (bytes [K,C], counts, n_gt, ap [C], summary, tables)."""
    C = preds.shape[1]
    whitelist_ids = [c for c in whitelist_ids if c <= num_classes]
    t = tables(metadata, names, groundtruth, excluded, whitelist_ids, C, mutant)
    xyxy = np.ascontiguousarray(boxes[:, 1:5], dtype=np.float32)
    by, counts, _ = match(xyxy, C, t["grp_off"], t["det_rows"], t["grp_image"], t["gt_off"], t["gt_class"], t["gt_boxes"],
                          t["whitelist"], scores=preds, mutant=mutant)
    ap, summary, _ = voc_ap(preds, by, t["n_gt"], mutant=mutant)
    return by, counts, t["n_gt"], ap, summary, t
