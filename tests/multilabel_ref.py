"""TEST INFRASTRUCTURE: numpy restatement, in float64, of csrc/multilabel.hip (focus_bce_rows, focus_view_accumulate_dense,
focus_average_precision), written from the contract in include/focus_amd.h, with the bounds the tests hold the kernels to.
Average precision is restated twice: by counting, in the kernel's order of summation, and by sorting and cumulating, which
shares nothing with the first but the definition.  `mutant` switches one rule to a plausible wrong one;
tests/test_multilabel_ref_cpu.py shows that the fixture's inputs tell each of them apart.

The bounds (u32 = 2^-24 and u64 = 2^-53 are the unit roundoffs of fp32 and fp64):

BCE.  The kernel evaluates the stated formula in fp32 from fp32 inputs; the twin evaluates it in fp64 from the same inputs.
  logits: e = (max(x,0) - x y) + log1p(exp(-|x|)).  x y rounds once (u32 |x y|); exp is good to 1 ulp = 2 u32 and log1p, whose
  condition number is at most 1 there, to 2 ulp = 4 u32, together 6 u32 log1p(.); the subtraction and the addition round once
  each, at most u32 (max(x,0) + |x y| + log1p(.)) each.  With A = max(x,0) + |x y| + log1p(exp(-|x|)) that is at most 8 u32 A.
  probs: e = -(y L1 + (1 - y) L0) with L1 = max(log x, -100), L0 = max(log1p(-x), -100).  log and log1p are good to 2 ulp
  = 4 u32 (the clamp is 1-Lipschitz), 1 - y and each product round once, the sum once: at most 8 u32 A with A = |y L1| + |(1-y) L0|.
  row: thread t adds ceil(C / 256) elements one after another, then 8 halving steps: at most d = ceil(C / 256) + 8 roundings
  on any path, each at most u32 times the sum of |e| <= sum of A.  Row bound: 1.01 (8 + d) u32 sum A + C 2^-126 (a result under
  the normal range is rounded to a multiple of 2^-149 or flushed).
  dx logits: g = s - y, s = (x >= 0 ? 1 : t) / (1 + t), t = exp(-|x|): t 2 u32, the sum and the correctly rounded quotient
  u32 each: s to 4 u32 s; the subtraction u32 |s - y|; the scale u32.  Bound |gs| u32 (4 s + 2 |s - y|) 1.01 + |gs| 2^-126.
  dx probs: g = (x - y) / max((1 - x) x, 1e-12f): five roundings, each relative u32, and max is 1-Lipschitz:
  1.01 . 6 u32 |dx| + |gs| 2^-126.
  A fast intrinsic is used nowhere (expf, logf, log1pf are the library's), so no term for one.

AP.  Both sides get the same integers; what differs is the float64 arithmetic on them.
  scikit-learn: recall_k = tps_k / P (u64), the step recall_k - recall_(k-1) from two such values (2 u64 + u64 |step|), times
  the precision (u64) and that itself a quotient (u64): at most 2 u64 + 3 u64 |step| per threshold; T <= N thresholds and
  steps summing to 1: (2 T + 3) u64; numpy's pairwise sum of T terms that sum to at most 1: (log2 T + 1) u64.  At most
  (2 N + log2 N + 4) u64 <= 6 N u64.
  kernel: each quotient TP / CNT u64; per tile 8 halving steps, then ceil(N / 256) sequential adds, then the division: at
  most (10 + N / 256) u64 relative, AP <= 1: <= 11 N u64.
  Together 17 N u64, stated as AP_K N 2^-53 with AP_K = 20.  The mean over C classes adds (C + 1) u64 on each side."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -126
AP_K = 20
MUTANTS = ("gt_count", "index_ties", "divide_by_n", "keep_zero_classes", "no_clamp", "unstable_log")
BAD_LABEL, BAD_SCORE, NO_CLASS = 1, 2, 4


# ---- BCE ------------------------------------------------------------------------------------------------------------------
def bce_elements(x, y, mode, dtype=np.float64, mutant=None):
    """(e, A, g): the elements, the magnitudes their error is measured against, and de/dx, every operation in `dtype`."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    one = dtype(1)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if mode == "logits":
            t = np.exp(-np.abs(x))
            if mutant == "unstable_log":
                sp = np.log(one + np.exp(x))                                 # softplus the naive way: overflows for large x
                e = sp - x * y
            else:
                sp = np.log1p(t)
                e = (np.maximum(x, 0) - x * y) + sp
            A = np.maximum(x, 0) + np.abs(x * y) + np.log1p(t)
            s = np.where(x >= 0, one, t) / (one + t)
            g = s - y
            return e.astype(dtype), A, g.astype(dtype), s
        lo = dtype(-np.inf) if mutant == "no_clamp" else dtype(-100)
        l1, l0 = np.maximum(np.log(x), lo), np.maximum(np.log1p(-x), lo)
        with np.errstate(invalid="ignore"):
            e = -(y * l1 + (one - y) * l0)
        A = np.abs(y * np.maximum(np.log(x), dtype(-100))) + np.abs((one - y) * np.maximum(np.log1p(-x), dtype(-100)))
        g = (x - y) / np.maximum((one - x) * x, dtype(np.float32(1e-12)))
        return e.astype(dtype), A, g.astype(dtype), None


def bce_rows(x, y, mode, grad_scale=1.0):
    """fp64: (loss_rows [R], dx [R,C], row bound [R], dx bound [R,C]) for fp32 inputs x, y [R,C]; grad_scale is an fp32
    argument of the entry point, so it is rounded to fp32 first, like x and y."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    grad_scale = float(np.float32(grad_scale))
    C = x.shape[1]
    e, A, g, s = bce_elements(x, y, mode)
    d = -(-C // 256) + 8
    row_bound = 1.01 * (8 + d) * U32 * A.sum(axis=1) + C * TINY32
    gs = abs(float(grad_scale))
    if mode == "logits":
        dx_bound = gs * U32 * (4 * s + 2 * np.abs(g)) * 1.01 + gs * TINY32
    else:
        dx_bound = 1.01 * 6 * U32 * gs * np.abs(g) + gs * TINY32
    return e.sum(axis=1), float(grad_scale) * g, row_bound, dx_bound


def loss_bound(rows, row_bound, grad_scale):
    """The operator on top of the rows: R row sums added in fp32 (at most R roundings of a running sum that never exceeds
    the sum of |rows|), one scaling, one rounding of the result."""
    return abs(grad_scale) * (row_bound.sum() + (len(rows) + 2) * U32 * np.abs(rows).sum() * 1.01)


def bce_rows_fp32(x, y, mode, mutant=None):
    """The row sums with every operation in fp32 and the kernel's order: thread t adds t, t + 256, ..., then the halving."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    R, C = x.shape
    e = bce_elements(x, y, mode, dtype=np.float32, mutant=mutant)[0]
    pad = np.zeros((R, -(-C // 256) * 256), dtype=np.float32)
    pad[:, :C] = e
    acc = np.zeros((R, 256), dtype=np.float32)
    for k in range(pad.shape[1] // 256):
        acc = (acc + pad[:, 256 * k:256 * k + 256]).astype(np.float32)
    return halving_sum(acc)


def halving_sum(v):
    """[..., 256] -> [...]: slot s += slot s + h for h = 128, 64, ..., 1, in the array's own type."""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = (v[..., :h] + v[..., h:]).astype(v.dtype)
    return v[..., 0]


# ---- the dense view fold ---------------------------------------------------------------------------------------------------
def view_accumulate_dense(preds, clip_ids, labels, num_clips, video_preds, video_labels, clip_count, flag, mode="sum"):
    """In place, clip by clip in row order: the loop of TestMeter.update_stats(multi_label=True) with the assertion turned
    into bit 0 of flag and a clip id out of range into bit 1.  preds are float32 values (bf16 ones widened)."""
    preds, labels = np.asarray(preds, dtype=np.float32), np.asarray(labels, dtype=np.float32)
    nv = video_preds.shape[0]
    for i, cid in enumerate(np.asarray(clip_ids).tolist()):
        if cid < 0 or cid >= nv * num_clips:
            flag[0] |= 2
            continue
        v = cid // num_clips
        if (video_labels[v] > 0).any() and not np.array_equal(video_labels[v], labels[i]):
            flag[0] |= 1
        video_labels[v] = labels[i]
        if mode == "sum":
            video_preds[v] = (video_preds[v] + preds[i]).astype(np.float32)
        else:
            p = preds[i]
            video_preds[v] = np.where(np.isnan(p) | (p > video_preds[v]), p, video_preds[v])
        clip_count[v] += 1


# ---- average precision -----------------------------------------------------------------------------------------------------
def ap_counts(s, y, mutant=None):
    """(CNT_i, TP_i) for every row i of one class: integers."""
    s = np.asarray(s, dtype=np.float32)
    pos = np.asarray(y) == 1
    ge = s[None, :] >= s[:, None]                                            # [i, j]: s_j >= s_i
    if mutant == "index_ties":                                               # ties broken by index: j counts only if j <= i
        idx = np.arange(s.size)
        ge = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] <= idx[:, None]))
    cnt = ge.sum(axis=1)
    if mutant == "gt_count":
        cnt = (s[None, :] > s[:, None]).sum(axis=1) + 1
    return cnt.astype(np.int64), (ge & pos[None, :]).sum(axis=1).astype(np.int64)


def average_precision_counting(scores, labels, mutant=None):
    """The kernel's form and order -> (ap [C] f64, npos [C] i64, summary [2] f64, flag int)."""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.float32)
    N, C = scores.shape
    ap, npos, flag = np.zeros(C), np.zeros(C, dtype=np.int64), 0
    tiles = -(-N // 256)
    for c in range(C):
        s, y = scores[:, c], labels[:, c]
        npos[c] = int((y != 0).sum())
        if npos[c] == 0 and mutant != "keep_zero_classes":
            continue
        if ((y != 0) & (y != 1)).any():
            flag |= BAD_LABEL
        if not np.isfinite(s).all():
            flag |= BAD_SCORE
        cnt, tp = ap_counts(s, y, mutant)
        q = np.zeros(tiles * 256)
        ok = (y == 1) & (cnt > 0)
        q[:N][ok] = tp[ok].astype(np.float64) / cnt[ok].astype(np.float64)
        total = 0.0
        for part in halving_sum(q.reshape(tiles, 256)):                      # the tiles in ascending order
            total = total + part
        den = N if mutant == "divide_by_n" else npos[c]
        ap[c] = total / float(den) if den > 0 else 0.0
    kept = npos > 0 if mutant != "keep_zero_classes" else np.ones(C, dtype=bool)
    total = 0.0
    for c in range(C):
        if kept[c]:
            total = total + ap[c]
    nk = int(kept.sum())
    if nk == 0:
        flag |= NO_CLASS
    return ap, npos, np.array([total / nk if nk else 0.0, float(nk)]), flag


def average_precision_sorting(s, y):
    """One class, by definition: thresholds are the distinct scores in descending order; at each, precision = positives at or
    above it / rows at or above it, and AP = sum of precision x (share of the positives that sit exactly at it)."""
    s, pos = np.asarray(s, dtype=np.float32), np.asarray(y) == 1
    order = np.argsort(-s.astype(np.float64), kind="stable")
    s, pos = s[order], pos[order]
    last = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]                  # the last row of every run of equal scores
    tp = np.cumsum(pos)[last].astype(np.float64)
    n = (last + 1).astype(np.float64)
    here = np.diff(np.r_[0.0, tp])
    return float(np.sum(here * (tp / n)) / tp[-1])


def get_map_twin(scores, labels, mutant=None):
    """What get_map returns, from the counting form: 0.0 where scikit-learn raises."""
    _, _, summary, flag = average_precision_counting(scores, labels, mutant)
    return 0.0 if flag & (BAD_SCORE | NO_CLASS) else float(summary[0])


def ap_bound(N):
    return AP_K * N * U64


def map_bound(N, C):
    return ap_bound(N) + 2 * (C + 1) * U64
