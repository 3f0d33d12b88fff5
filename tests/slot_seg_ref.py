"""TEST INFRASTRUCTURE: plain numpy / torch restatement of csrc/slot_segments.hip (focus_slot_segments, focus_slot_boxes,
focus_seg_contingency) and of the per-clip selection rule, for the CPU fixture tests and the GPU tests.  Written from the
contract in include/focus_amd.h, loop by loop where a vectorised form would hide a rule.  The `mutant` argument switches
one rule to a plausible wrong one; tests/test_slot_seg_ref_cpu.py shows that the fixture tells each of them apart."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "slot_boxes.npz")

# name -> (B, T, He, We, K, sy, sx, levels): the recorded cases of tests/golden/slot_boxes.npz (tests/make_slot_boxes_golden.py
# searches a seed per case at which every slot owns a cell in every frame); "thin" is thin_attn() below
CASES = {
    "square4": (2, 3, 8, 8, 5, 4, 4, None),
    "wide": (1, 2, 6, 10, 4, 2, 4, None),
    "eleven": (1, 2, 16, 16, 11, 1, 1, None),
    "ties": (1, 2, 8, 8, 4, 2, 2, 4),
    "thin": (1, 1, 4, 10, 3, 5, 2, None),
}
MUTANTS = ("no_plus_s", "ties_high", "lt_eps", "area_order", "keep_background")


def make_attn(B, T, He, We, K, seed, levels=None):
    """Blocky fp32 scores [B,T,N,K]: every slot owns a rectangle of the grid (so boxes are not all the whole frame) under
    noise; `levels` quantises the scores to that many values, which makes exact ties."""
    g = np.random.RandomState(seed)
    a = g.rand(B, T, He, We, K).astype(np.float32)
    for b in range(B):
        for t in range(T):
            for k in range(K):
                y0, x0 = g.randint(0, He), g.randint(0, We)
                y1, x1 = g.randint(y0, He) + 1, g.randint(x0, We) + 1
                a[b, t, y0:y1, x0:x1, k] += np.float32(0.75)
    if levels:
        a = np.floor(a * levels / 2).astype(np.float32) / np.float32(levels)
    return a.reshape(B, T, He * We, K)


def thin_attn():
    """Case "thin" (4x10 grid, 20x20 frame): slot 1 owns column 0 alone, so its box is 2 of 20 pixels wide and
    w = fl(1/20) - 0 is exactly the fp32 0.05 the "no object" rule compares with (<= zeroes it, < would keep it); slot 2
    owns columns 1-2 (pixels 2..5: w = 5/20 - 2/20), slot 0 the rest."""
    a = np.zeros((1, 1, 4, 10, 3), dtype=np.float32)
    a[..., 0] = 0.5
    a[:, :, :, 0, 1] = 1.0
    a[:, :, :, 1:3, 2] = 1.0
    return a.reshape(1, 1, 40, 3)


def argmax_map(attn, mutant=None):
    """attn [B,T,N,K] (numpy, any float type) -> uint8 [B,T,N]: the first of equal maxima."""
    attn = np.asarray(attn, dtype=np.float64)                 # exact for fp32 and bf16 values: only the order matters
    K = attn.shape[-1]
    if mutant == "ties_high":
        return (K - 1 - np.argmax(attn[..., ::-1], axis=-1)).astype(np.uint8)
    return np.argmax(attn, axis=-1).astype(np.uint8)          # numpy: the first of equal maxima


def stats_of(seg, He, We, K):
    """seg [B,T,N] -> int32 [B,T,K,5] = (count, xmin, ymin, xmax, ymax) per frame and slot; (0, We, He, -1, -1) if absent."""
    seg = np.asarray(seg)
    B, T, N = seg.shape
    assert N == He * We
    ys, xs = np.divmod(np.arange(N), We)
    stats = np.zeros((B, T, K, 5), dtype=np.int32)
    for k in range(K):
        m = seg == k
        stats[:, :, k, 0] = m.sum(-1)
        stats[:, :, k, 1] = np.where(m, xs, We).min(-1)
        stats[:, :, k, 2] = np.where(m, ys, He).min(-1)
        stats[:, :, k, 3] = np.where(m, xs, -1).max(-1)
        stats[:, :, k, 4] = np.where(m, ys, -1).max(-1)
    return stats


def segments(attn, He, We, mutant=None):
    """focus_slot_segments: attn [B,T,N,K] -> (seg uint8 [B,T,N], stats int32 [B,T,K,5])."""
    seg = argmax_map(attn, mutant)
    return seg, stats_of(seg, He, We, np.asarray(attn).shape[-1])


def select(stats, O, drop_largest=True, mutant=None):
    """stats [B,T,K,5] -> list over clips of the kept slots in output order."""
    B, T, K, _ = stats.shape
    out = []
    for b in range(B):
        area = stats[b, :, :, 0].astype(np.int64).sum(axis=0)
        cand = list(range(K))
        if drop_largest and mutant != "keep_background":
            cand.remove(max(cand, key=lambda k: (area[k], -k)))
        cand = [k for k in cand if area[k] > 0]
        by_area = sorted(cand, key=lambda k: (-area[k], k))[:O]
        out.append(by_area if mutant == "area_order" else sorted(by_area))
    return out


def pixel_boxes(stats, sy, sx, mutant=None):
    """stats [...,5] -> fp32 [...,4] xyxy pixel boxes of the nearest-upsampled masks (rows of empty slots are garbage)."""
    s = stats.astype(np.int64)
    px = sx - 1 if mutant != "no_plus_s" else 0
    py = sy - 1 if mutant != "no_plus_s" else 0
    return np.stack([s[..., 1] * sx, s[..., 2] * sy, s[..., 3] * sx + px, s[..., 4] * sy + py], axis=-1).astype(np.float32)


def to_orvit(px, H, W, mutant=None):
    """datasets/utils.boxes_to_orvit_format restated in numpy fp32, one rounding per step: px [...,4] xyxy -> cxcywh."""
    px = np.asarray(px, dtype=np.float32)
    x0, x1 = px[..., 0] / np.float32(W), px[..., 2] / np.float32(W)
    y0, y1 = px[..., 1] / np.float32(H), px[..., 3] / np.float32(H)
    x0, y0, x1, y1 = (np.clip(v, np.float32(0), np.float32(1)) for v in (x0, y0, x1, y1))
    out = np.stack([(x0 + x1) / np.float32(2), (y0 + y1) / np.float32(2), x1 - x0, y1 - y0], axis=-1).astype(np.float32)
    eps = np.float32(0.05)
    empty = (out[..., 2:] < eps).any(-1) if mutant == "lt_eps" else (out[..., 2:] <= eps).any(-1)
    out[empty] = 0
    return out


def boxes(stats, He, We, H, W, O, drop_largest=True, mutant=None):
    """focus_slot_boxes: stats [B,T,K,5] -> (boxes fp32 [B,T,O,4], slot_ids int32 [B,O])."""
    assert H % He == 0 and W % We == 0
    B, T, K, _ = stats.shape
    rows = to_orvit(pixel_boxes(stats, H // He, W // We, mutant), H, W, mutant)            # [B,T,K,4]
    out = np.zeros((B, T, O, 4), dtype=np.float32)
    ids = np.full((B, O), -1, dtype=np.int32)
    for b, kept in enumerate(select(stats, O, drop_largest, mutant)):
        for o, k in enumerate(kept):
            ids[b, o] = k
            for t in range(T):
                if stats[b, t, k, 0] > 0:
                    out[b, t, o] = rows[b, t, k]
    return out, ids


def contingency(seg, truth, He, We, K, first_segment=1):
    """focus_seg_contingency: seg uint8 [B,T,N], truth [B,T,S,1,H,W] (non-zero = member) -> int32 [B,S-first,K]."""
    seg, truth = np.asarray(seg), np.asarray(truth)
    B, T, S, _, H, W = truth.shape
    sy, sx = H // He, W // We
    assert sy * He == H and sx * We == W
    up = seg.reshape(B, T, He, We).repeat(sy, axis=2).repeat(sx, axis=3)                    # [B,T,H,W]
    table = np.zeros((B, S - first_segment, K), dtype=np.int32)
    for s in range(first_segment, S):
        member = truth[:, :, s, 0] != 0
        for k in range(K):
            table[:, s - first_segment, k] = (member & (up == k)).sum(axis=(1, 2, 3))
    return table


def upsampled_onehot(seg, He, We, K, sy, sx):
    """seg [B,T,N] -> float32 one-hot masks [B,T,K,He*sy,We*sx], nearest-upsampled like STEVE._slots does."""
    B, T, N = seg.shape
    one = (seg.reshape(B, T, 1, He, We) == np.arange(K).reshape(1, 1, K, 1, 1)).astype(np.float32)
    return one.repeat(sy, axis=3).repeat(sx, axis=4)


def ari(table):
    from focus_amd.slowfast.utils import metrics
    return metrics.ari_from_tables(torch.from_numpy(np.asarray(table)))
