"""Slot masks -> FG-ARI tables and ORViT boxes on the device (csrc/slot_segments.hip) against the path of the parent commit
on the same device.

    python tools/slot_segments_bench.py [--rounds 9] [--iters 5] [--no-model] [--out FILE]

Shape: B=8, T=24, K=11 slots, N=4096 cells (64x64), 128x128 frames, S=24 truth segments (segment 0 = background).

1. The three kernels alone, on a synthetic bf16 slot attention [B,T,N,K] and uint8 truth: time per call, the algorithm's
   bytes (attn read once + seg and stats written; stats read + boxes written; truth read once + seg read once + table
   written), bytes per second and that as a share of the 8 TB/s HBM peak.  The working set (35 MB, 75 MB) fits the 256 MiB
   Infinity Cache, so a share near or above what HBM sustains (about 6.3 TB/s) says the data came from the cache.
2. The tail of slot_eval_epoch's body from the slot update's attention on, both ways: the parent's (upsample to
   [B,T,K,1,H,W] fp32, attns_vis, evaluate_ari's arg-max + float64 one-hot + float64 matmul) against
   ops.slot_segments + metrics.evaluate_ari_segments.  The scores are compared first.
3. Boxes from the same attention: the parent's only route (upsample, arg-max, one-hot masks, box_ops.masks_to_boxes,
   datasets.utils.boxes_to_orvit_format through the host) against ops.slot_segments + ops.slot_boxes.
4. Unless --no-model: slot_eval_epoch's whole body on the STEVE model of bench.py's model step (bf16 storage), encode +
   evaluate_ari against segment + evaluate_ari_segments, and the peak memory of each.

Sides are timed as whole calls with device events after a warm-up, alternating round by round; medians with the spread."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.datasets.utils import boxes_to_orvit_format  # noqa: E402
from focus_amd.slowfast.utils import box_ops, metrics  # noqa: E402

B, T, K, HE, WE, H, W, S, O = 8, 24, 11, 64, 64, 128, 128, 24, 5
HBM_PEAK = 8.0e12


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us per call


def alternate(fns, rounds, iters):
    for f in fns:
        timed(f, 2)
    out = [[] for _ in fns]
    for _ in range(rounds):
        for o, f in zip(out, fns):
            o.append(timed(f, iters))
    return out


def line(name, t):
    return "    %-34s median %10.1f us   min %10.1f   max %10.1f" % (name, statistics.median(t), min(t), max(t))


def parent_masks(attns, video_hw):
    """STEVE._slots' tail: [B,T,N,K] -> [B,T,K,1,H,W] fp32."""
    b, t, n, k = attns.shape
    return attns.float().transpose(-1, -2).reshape(b, t, k, 1, HE, WE) \
        .repeat_interleave(video_hw[0] // HE, dim=-2).repeat_interleave(video_hw[1] // WE, dim=-1)


def parent_eval_tail(attns, video, truth):
    masks = parent_masks(attns, video.shape[-2:])
    attns_vis = video.unsqueeze(2) * masks + (1.0 - masks)              # encode() builds it whether or not it is read
    del attns_vis
    return metrics.evaluate_ari(truth.permute(0, 2, 1, 3, 4, 5)[:, 1:].flatten(start_dim=2),
                                masks.permute(0, 2, 1, 3, 4, 5).flatten(start_dim=2))


def fused_eval_tail(attns, video, truth):
    seg, _ = ops.slot_segments(attns, HE, WE)
    return metrics.evaluate_ari_segments(truth, seg.view(B, T, HE, WE), K)


def parent_boxes(attns, video):
    """The O largest non-background slots' boxes by the parent's tools: masks on the device, boxes through the host."""
    masks = parent_masks(attns, video.shape[-2:])[:, :, :, 0]           # B,T,K,H,W
    am = masks.argmax(dim=2, keepdim=True)
    onehot = torch.zeros_like(masks).scatter_(2, am, 1.0)
    area = onehot.sum(dim=(1, 3, 4))                                    # B,K
    px = box_ops.masks_to_boxes(onehot.flatten(end_dim=2)).reshape(B, T, K, 4)
    rows = boxes_to_orvit_format(px, H, W).to(attns.device)             # zeroes thin boxes; empty masks give zero rows too
    area[torch.arange(B), area.argmax(dim=1)] = -1                      # drop the background
    order = torch.sort(torch.topk(area, O, dim=1).indices, dim=1).values
    return torch.gather(rows, 2, order.view(B, 1, O, 1).expand(B, T, O, 4))


def fused_boxes(attns, video):
    _, stats = ops.slot_segments(attns, HE, WE)
    return ops.slot_boxes(stats, HE, WE, H, W, O)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slot_segments_bench: needs the MI355X (timings from a CPU say nothing about it)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("B=%d T=%d K=%d N=%d (%dx%d) frames %dx%d S=%d O=%d; %d rounds x %d calls, alternated" % (
        B, T, K, HE * WE, HE, WE, H, W, S, O, args.rounds, args.iters))
    g = torch.Generator().manual_seed(0)
    # blocky scores: every slot has a rectangle of its own per clip, under noise (objects, not salt and pepper)
    score = torch.rand(B, T, HE, WE, K, generator=g)
    for b in range(B):
        for k in range(K):
            y0, x0 = int(torch.randint(0, HE - 8, (1,), generator=g)), int(torch.randint(0, WE - 8, (1,), generator=g))
            score[b, :, y0:y0 + 8 + 2 * k, x0:x0 + 8 + 2 * k, k] += 0.8
    score[..., 0] += 0.45                                               # slot 0: the background
    attns = torch.softmax(score.reshape(B, T, HE * WE, K) * 8, dim=-1).to(torch.bfloat16).to(dev)
    video = torch.rand(B, T, 3, H, W, generator=g).to(dev)
    lab = torch.randint(0, S, (B, T, H // 8, W // 8), generator=g).repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    truth = torch.nn.functional.one_hot(lab, S).permute(0, 1, 4, 2, 3).unsqueeze(3).to(torch.uint8).contiguous().to(dev)

    say("1. kernels alone (bf16 attention, uint8 truth)")
    seg, stats = ops.slot_segments(attns, HE, WE)
    nb = {"focus_slot_segments": attns.numel() * 2 + seg.numel() + stats.numel() * 4,
          "focus_slot_boxes": stats.numel() * 4 + B * T * O * 16 + B * O * 4,
          "focus_seg_contingency": B * T * (S - 1) * H * W + seg.numel() + B * (S - 1) * K * 4}
    # through the C ABI into preallocated outputs: the operators' torch.empty calls would cost more host time than the kernels run
    L, st = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    boxes, ids = ops.slot_boxes(stats, HE, WE, H, W, O)
    table = ops.seg_contingency(seg, truth, HE, WE, K)
    fns = {"focus_slot_segments": lambda: L.focus_slot_segments(ptr(attns), _lib.BF16, B, T, HE, WE, K, ptr(seg), ptr(stats), st),
           "focus_slot_boxes": lambda: L.focus_slot_boxes(ptr(stats), B, T, K, HE, WE, H, W, O, 1, ptr(boxes), ptr(ids), st),
           "focus_seg_contingency": lambda: L.focus_seg_contingency(ptr(seg), ptr(truth), 0, B, T, S, H, W, HE, WE, K, 1,
                                                                    ptr(table), st)}
    for name, f in fns.items():
        t = alternate([f], args.rounds, max(args.iters, 20))[0]
        med = statistics.median(t)
        say(line(name, t))
        say("      %.2f MB algorithmic -> %.3f TB/s = %.1f %% of the 8 TB/s HBM peak" % (
            nb[name] / 1e6, nb[name] / med / 1e6, 100 * nb[name] / (med * 1e-6) / HBM_PEAK))

    say("2. slot_eval_epoch's body from the attention on")
    a, f = parent_eval_tail(attns, video, truth), fused_eval_tail(attns, video, truth)
    say("    FG-ARI parent %.15f fused %.15f equal: %s" % (a, f, a == f))
    tp, tf = alternate([lambda: parent_eval_tail(attns, video, truth), lambda: fused_eval_tail(attns, video, truth)],
                       args.rounds, args.iters)
    say(line("parent: upsample + evaluate_ari", tp))
    say(line("fused: segments + contingency", tf))
    r = [p / q for p, q in zip(tp, tf)]
    say("    parent / fused per round: median %.1fx, min %.1fx, max %.1fx" % (statistics.median(r), min(r), max(r)))
    for name, fn in (("parent", parent_eval_tail), ("fused", fused_eval_tail)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(attns, video, truth)
        torch.cuda.synchronize()
        say("    %s peak memory above the inputs: %.1f MB" % (name, (torch.cuda.max_memory_allocated() - base) / 1e6))

    say("3. orvit_bboxes [B,T,O,4] from the attention")
    pb, fb = parent_boxes(attns, video), fused_boxes(attns, video)
    say("    boxes bit-equal: %s" % bool(torch.equal(pb, fb)))
    tp, tf = alternate([lambda: parent_boxes(attns, video), lambda: fused_boxes(attns, video)], args.rounds, args.iters)
    say(line("parent: masks_to_boxes via host", tp))
    say(line("fused: segments + slot_boxes", tf))
    r = [p / q for p, q in zip(tp, tf)]
    say("    parent / fused per round: median %.1fx, min %.1fx, max %.1fx" % (statistics.median(r), min(r), max(r)))

    if not args.no_model:
        say("4. slot_eval_epoch's whole body on the STEVE model (bf16 storage), B=%d" % B)
        from focus_amd.slowfast.config.defaults import get_cfg
        from focus_amd.slowfast.models import MODEL_REGISTRY
        cfg = get_cfg()
        cfg.MODEL.MODEL_NAME = "STEVE"
        cfg.NUM_GPUS = 1
        cfg.TRAIN.MIXED_PRECISION = True
        sl = cfg.SLOTS
        sl.NUM_ITERS, sl.NUM_SLOTS, sl.CNN_HID_SIZE, sl.SIZE, sl.DIM, sl.MLP_HID_SIZE, sl.IMG_SIZE, sl.VOCAB_SIZE = 3, K, 64, 192, 192, 768, H, 4096
        sl.NUM_PREDICTOR_BLOCKS, sl.NUM_PREDICTOR_HEADS, sl.PREDICTOR_DROPOUT = 1, 4, 0.0
        sl.DECODER.DIM, sl.DECODER.NUM_BLOCKS, sl.DECODER.NUM_HEADS, sl.DECODER.DROPOUT = 192, 8, 4, 0.1
        torch.manual_seed(0)
        m = MODEL_REGISTRY.get("STEVE")(cfg).to(dev).eval()

        def parent_body():
            _, _, pm = m.encode(video)
            return metrics.evaluate_ari(truth.permute(0, 2, 1, 3, 4, 5)[:, 1:].flatten(start_dim=2),
                                        pm.permute(0, 2, 1, 3, 4, 5).flatten(start_dim=2))

        def fused_body():
            _, sg, _ = m.segment(video)
            return metrics.evaluate_ari_segments(truth, sg, K)

        with torch.no_grad():
            torch.manual_seed(1)
            a = parent_body()
            torch.manual_seed(1)
            f = fused_body()
            say("    FG-ARI parent %.15f fused %.15f equal: %s" % (a, f, a == f))
            tp, tf = alternate([parent_body, fused_body], max(3, args.rounds // 2), 2)
            say(line("parent: encode + evaluate_ari", [t / 1e3 for t in tp]).replace(" us", " ms"))
            say(line("fused: segment + ari_segments", [t / 1e3 for t in tf]).replace(" us", " ms"))
            r = [p / q for p, q in zip(tp, tf)]
            say("    parent / fused per round: median %.2fx, min %.2fx, max %.2fx" % (statistics.median(r), min(r), max(r)))
            for name, fn in (("parent", parent_body), ("fused", fused_body)):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                say("    %s peak memory above the model and inputs: %.1f MB" % (name, (torch.cuda.max_memory_allocated() - base) / 1e6))
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
