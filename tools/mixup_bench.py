"""Mixup / CutMix on the device: focus_mixup_blend and focus_cutmix_paste (csrc/mixup.hip) against the reference's own ATen
sequences on the same device tensors, at the batch of the shipped ORViT configs.

    python tools/mixup_bench.py [--rounds 15] [--iters 20] [--out FILE]

Workload: a [8,3,16,224,224] batch in fp32 and in bf16.  Blend: `ops.mixup_blend_(x, lam)` against
`f = x.flip(0).mul_(1 - lam); x.mul_(lam).add_(f)` (mixup.py:179-180).  Paste: `ops.cutmix_paste_` against
`x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]` (mixup.py:177) for the centred quarter-frame box.  The outputs of the
two sides are compared bit for bit at this size first.  Both sides are timed as whole calls with device events after a
warm-up, alternating round by round; the spread over the rounds is printed beside the medians.  Each is timed twice: on one
buffer again and again (77 / 39 MB: it stays in the 256 MiB Infinity Cache, as a batch the sampler has just written may), and
rotating over enough buffers that every call finds its batch in HBM.  Bytes are the algorithm's: one read and one write of
what the operation touches."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import ops  # noqa: E402

SHAPE = (8, 3, 16, 224, 224)
LAM = 0.37
BOX = (56, 168, 56, 168)                  # yl, yh, xl, xh: a quarter of the frame
ROTATE_BYTES = 640 << 20                  # the buffers of one side together, well past the 256 MiB Infinity Cache


def aten_blend(x):
    f = x.flip(0).mul_(1.0 - LAM)
    x.mul_(LAM).add_(f)


def hip_blend(x):
    ops.mixup_blend_(x, LAM)


def aten_paste(x):
    yl, yh, xl, xh = BOX
    x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]


def hip_paste(x):
    ops.cutmix_paste_(x, *BOX)


def timed(fn, bufs, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(bufs[i % len(bufs)])
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_bench: needs the MI355X (timings from a CPU say nothing about it)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("batch %s, lam %.2f, box y %d:%d x %d:%d; %d rounds x %d calls, alternated" % ((list(SHAPE), LAM) + BOX + (args.rounds, args.iters)))
    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        g = torch.Generator().manual_seed(1)
        base = torch.randn(*SHAPE, generator=g).to(dtype).cuda()
        nbytes = base.numel() * base.element_size()
        nrot = -(-ROTATE_BYTES // nbytes)
        for op, aten, hip, touched in (("blend", aten_blend, hip_blend, nbytes), ("paste", aten_paste, hip_paste, nbytes // 4)):
            xa, xh = base.clone(), base.clone()
            aten(xa)
            hip(xh)
            say("%s %s: outputs bit-equal at this size: %s" % (op, dname, bool(torch.equal(xa, xh))))
            for where, n in (("one buffer (cache-resident)", 1), ("%d buffers in rotation (HBM)" % nrot, nrot)):
                ba, bh = [base.clone() for _ in range(n)], [base.clone() for _ in range(n)]
                for _ in range(2):
                    timed(aten, ba, max(n, 5))
                    timed(hip, bh, max(n, 5))
                ta, th = [], []
                for _ in range(args.rounds):
                    ta.append(timed(aten, ba, args.iters))
                    th.append(timed(hip, bh, args.iters))
                ratio = [a / h for a, h in zip(ta, th)]
                say("  %s" % where)
                say("    HIP kernel      median %8.1f us   min %8.1f   max %8.1f   (%.2f TB/s of 2 x %.1f MB)" % (
                    statistics.median(th), min(th), max(th), 2 * touched / statistics.median(th) / 1e6, touched / 1e6))
                say("    ATen sequence   median %8.1f us   min %8.1f   max %8.1f" % (statistics.median(ta), min(ta), max(ta)))
                say("    ATen / HIP per round: median %.2fx, min %.2fx, max %.2fx" % (statistics.median(ratio), min(ratio), max(ratio)))
                del ba, bh
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
