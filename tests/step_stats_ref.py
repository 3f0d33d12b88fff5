"""TEST INFRASTRUCTURE: plain numpy restatement of csrc/step_stats.hip (focus_topk_stats, focus_view_accumulate), written
from the contract in include/focus_amd.h, loop by loop: the order rule, the mixup collapse with its single rounding, the
multitask counts, the scalar sums in double, and the per-clip accumulate with the conflict rule.  Logits are float32 arrays;
`bf16=True` says they hold bf16 values (the collapsed sum is then rounded to bf16).  The `mutant` argument switches one
rule to a plausible wrong one; tests/test_step_stats_ref_cpu.py shows that some case tells each of them apart."""
import numpy as np

MUTANTS = ("ties_high", "no_round", "keep_second", "either_head", "descending")
NI, NF = 16, 8
STEPS, SAMPLES, NAN, NAN_STEP, CORRECT = 0, 1, 2, 3, 4


def round_bf16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32; NaN stays NaN."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float32)


def magnitudes():
    """The 512 bf16-exact magnitudes (1 + m/128) 2^e, m < 128, e in {-1, 0, 1, 2}: distinct in fp32 and in bf16."""
    m = np.arange(128, dtype=np.float32)
    return np.concatenate([(1 + m / 128) * np.float32(2.0 ** e) for e in (-1, 0, 1, 2)]).astype(np.float32)


def tie_free_rows(B, V, seed):
    """[B,V] float32 rows of distinct bf16-exact values in random order with random signs (|x| distinct, so x distinct)."""
    g = np.random.RandomState(seed)
    mag = magnitudes()
    assert V <= mag.size
    rows = np.stack([g.permutation(mag)[:V] for _ in range(B)])
    return (rows * g.choice(np.float32([-1, 1]), size=rows.shape)).astype(np.float32)


def beats(x, i, y, j, mutant=None):
    xn, yn = bool(np.isnan(x)), bool(np.isnan(y))
    if xn != yn:
        return xn
    if mutant == "ties_high":
        return bool(x > y or (x == y and i > j))
    return bool(x > y or (x == y and i < j))


def _before(x, i, y, j, mutant):
    if np.isnan(x) and np.isnan(y):                      # several NaNs in a label row: the lowest index first
        return i < j
    return beats(x, i, y, j, mutant)


def greatest(row, skip=-1, mutant=None):
    best = -1
    for j in range(len(row)):
        if j != skip and (best < 0 or _before(row[j], j, row[best], best, mutant)):
            best = j
    return best


def row_rank(pred, label, bf16, mutant=None):
    """How many entries of the row beat the label's entry (-1: no label inside the row).  `label` is an index or a dense
    row, which is collapsed first."""
    pred = np.array(pred, dtype=np.float32)
    if np.ndim(label) == 1:
        first = greatest(label, mutant=mutant)
        second = greatest(label, skip=first, mutant=mutant)
        s = np.float32(pred[first]) + np.float32(pred[second])
        pred[first] = round_bf16(s) if bf16 and mutant != "no_round" else s
        if mutant != "keep_second":
            pred[second] = 0.0
        label = first
    label = int(label)
    if not 0 <= label < len(pred):
        return -1
    return sum(1 for j in range(len(pred)) if j != label and beats(pred[j], j, pred[label], label, mutant))


def new_acc():
    return np.zeros(NI, dtype=np.int64), np.zeros(NF, dtype=np.float64)


def topk_stats(acc_i, acc_f, preds=(), labels=(), ks=(1, 5), losses=(), batch=None, bf16=False, mutant=None):
    """Adds one batch into (acc_i, acc_f) in place, like the kernel.  preds / labels: tuples of one or two heads."""
    heads = len(preds)
    B = len(preds[0]) if heads else int(batch)
    if B <= 0:
        return
    bf = (bf16,) * heads if isinstance(bf16, bool) else tuple(bf16)
    for r in range(B):
        ranks = [row_rank(preds[h][r], labels[h][r], bf[h], mutant) for h in range(heads)]
        for j, k in enumerate(ks if heads else ()):
            ok = [0 <= x < k for x in ranks]
            for h in range(heads):
                acc_i[CORRECT + 4 * h + j] += ok[h]
            acc_i[CORRECT + 8 + j] += any(ok) if mutant == "either_head" else all(ok)
    steps = int(acc_i[STEPS])
    for i, l in enumerate(losses):
        if l is None:
            continue
        l = np.float64(np.float32(l))
        acc_f[i] = acc_f[i] + l
        acc_f[3 + i] = acc_f[3 + i] + l * np.float64(B)
    if len(losses) and losses[0] is not None and np.isnan(np.float32(losses[0])) and acc_i[NAN] == 0:
        acc_i[NAN] = 1
        acc_i[NAN_STEP] = steps
    acc_i[STEPS] = steps + 1
    acc_i[SAMPLES] += B


def view_accumulate(preds, clip_ids, labels, num_clips, video_preds, video_labels, clip_count, mode="sum", mutant=None):
    """Folds one batch into the tables in place and returns the flag bits it sets.  preds float32 [n,C] (bf16 values are
    exact in it).  Per video, the rows are taken in ascending row order starting from the table's row."""
    preds = np.asarray(preds, dtype=np.float32)
    n = len(preds)
    total = video_preds.shape[0] * num_clips
    flag = 0
    order = range(n - 1, -1, -1) if mutant == "descending" else range(n)
    for i in order:
        cid = int(clip_ids[i])
        if not 0 <= cid < total:
            flag |= 2
            continue
        v = cid // num_clips
        if video_labels[v] != 0 and video_labels[v] != labels[i]:
            flag |= 1
        video_labels[v] = labels[i]
        if mode == "sum":
            video_preds[v] = video_preds[v] + preds[i]                          # fp32, one rounding per clip
        else:
            p, a = preds[i], video_preds[v]
            video_preds[v] = np.where(np.isnan(p) | (p > a), p, a)
        clip_count[v] += 1
    return flag
