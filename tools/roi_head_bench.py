"""RoI head pooling, forward + backward: the fused ops.roi_head_pool against the composition of the existing ops
(mean over T in torch -> ops.roi_align_tokens -> ops.cell_amax) on the token stream [B, 1 + T*H*W, C].

  python tools/roi_head_bench.py [--rounds 20] [--inner 50] [--out profiles/roi_head_bench.txt]

Shapes: the AVA shape (B = 16 clips, T = 8, 7 x 7 map, C = 768, 3 boxes per clip, 7 x 7 bins, bf16) and the same with a 14 x 14
map.  The two arms alternate round by round; a round times `inner` forward + backward calls of one arm between two device
events.  Reported per shape: the median and the spread of the rounds of each arm, in how many rounds the fused arm was not
slower, the kernel launches of one forward + backward (counted by the profiler in a pass of its own) and the peak of temporary
device memory during one forward + backward (allocator peak above the live inputs; the outputs and x.grad are part of it in both
arms).  Needs the GPU: there is no CPU path."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from focus_amd import ops  # noqa: E402


def make(B, T, H, W, C, per_clip, crop, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1 + T * H * W, C, generator=g).to(dev).bfloat16().requires_grad_(True)
    K = B * per_clip
    xy = torch.rand(K, 2, generator=g) * 0.5
    wh = torch.rand(K, 2, generator=g) * 0.45 + 0.05
    idx = torch.arange(B).repeat_interleave(per_clip)[torch.randperm(K, generator=g)].float()
    rois = torch.cat([idx[:, None], xy * crop, (xy + wh) * crop], dim=1).to(dev)
    dp = torch.randn(K, C, generator=g).to(dev).bfloat16()
    return x, rois, dp


def fused(x, rois, dp, T, H, W, P, scale):
    y = ops.roi_head_pool(x, rois, T, H, W, P, P, scale, sampling_ratio=0, aligned=True, cls=1)
    y.backward(dp)
    return y


_SPLIT = {}


def composed(x, rois, dp, T, H, W, P, scale):
    B, _, C = x.shape
    if id(rois) not in _SPLIT:                                    # the box layout of roi_align_tokens, made once, not timed
        _SPLIT[id(rois)] = (rois[:, 1:].contiguous(), rois[:, 0].to(torch.int32))
    rois4, roi_img = _SPLIT[id(rois)]
    mean = x[:, 1:].reshape(B, T, H * W, C).mean(1)
    cells = ops.roi_align_tokens(mean, rois4, roi_img, H, W, P, P, scale, 0, True)
    y = ops.cell_amax(cells)
    y.backward(dp)
    return y


def timed(fn, args, x, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        x.grad = None
        fn(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                     # us per forward + backward


def launches(fn, args, x):
    from torch.profiler import ProfilerActivity, profile
    x.grad = None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(*args)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    return len(names), names


def temp_bytes(fn, args, x):
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "roi_head_bench.txt"))
    a = ap.parse_args()

    def save(lines):                                              # after every block: a later pass cannot lose the timings
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not torch.cuda.is_available():
        raise SystemExit("roi_head_bench: needs the GPU (no CPU path, no timing without one)")
    dev = torch.device("cuda:0")
    lines = ["RoI head pooling, forward + backward, bf16, %s; %d rounds x %d calls per arm, arms alternating; us per fwd+bwd"
             % (torch.cuda.get_device_name(0), a.rounds, a.inner),
             "(agreement: random inputs; the composition rounds the mean and the cells to bf16, so where two bins tie within that "
             "rounding the arms route a gradient through different bins -- tests/test_gpu_roi_head.py compares them on separated bins)"]
    for name, (B, T, H, W, C, per, P, crop) in (("AVA 16 x 8 x 7x7 x 768, 48 boxes", (16, 8, 7, 7, 768, 3, 7, 224.0)),
                                                 ("14x14 map 16 x 8 x 14x14 x 768, 48 boxes", (16, 8, 14, 14, 768, 3, 7, 224.0))):
        x, rois, dp = make(B, T, H, W, C, per, crop, dev)
        scale = H / crop
        args = (x, rois, dp, T, H, W, P, scale)
        ya = fused(*args).detach().float()
        ga = x.grad.float().clone()
        x.grad = None
        yb = composed(*args).detach().float()
        gb = x.grad.float().clone()
        lines.append("%s" % name)
        lines.append("  agreement  max |pooled| diff %.3e  max |dx| diff %.3e  (|pooled| max %.2f, |dx| max %.3e)" % (
            float((ya - yb).abs().max()), float((ga - gb).abs().max()), float(ya.abs().max()), float(ga.abs().max())))
        for fn in (fused, composed):                              # warm-up of both arms at this shape
            timed(fn, args, x, 10)
        tf, tc = [], []
        for _ in range(a.rounds):
            tf.append(timed(fused, args, x, a.inner))
            tc.append(timed(composed, args, x, a.inner))
        wins = sum(f <= c for f, c in zip(tf, tc))
        for label, t in (("fused", tf), ("composed", tc)):
            lines.append("  %-9s median %8.1f us   min %8.1f   max %8.1f" % (label, statistics.median(t), min(t), max(t)))
        lines.append("  fused not slower in %d of %d rounds; median ratio composed / fused %.2f" % (
            wins, a.rounds, statistics.median(tc) / statistics.median(tf)))
        save(lines)
        for label, fn in (("fused", fused), ("composed", composed)):
            try:
                n, names = launches(fn, args, x)
                ln = "%d" % n if n else "not measured (the profiler returned no device events)"
            except Exception as ex:                               # the profiler, not the measurement above
                ln = "not measured (%s)" % type(ex).__name__
            lines.append("  %-9s launches per fwd+bwd %s   temporary bytes (allocator peak) %d" % (label, ln, temp_bytes(fn, args, x)))
    save(lines)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
