"""The multi-label route on the device against the reference's host route.

    python tools/multilabel_bench.py [--rounds 5] [--out profiles/multilabel_bench.txt]

Four measurements; the two arms of each alternate round by round (A, B, A, B, ...) on one device, every round is a wall clock
around work that ends in a device synchronise, every round is printed, the medians are compared.

  1  get_map of a table that is on the device.  A: the reference's path, both tables .cpu().numpy() and scikit-learn's
     average_precision_score (the numpy restatement of it in meters.py where scikit-learn is absent; the header says which).
     B: meters.get_map on the device tensors (focus_average_precision and one small copy).  Two sizes: the Charades test
     set, 1863 x 157 with sparse positives, and a Cholec80-like tool table, 100000 x 7 with dense positives.
  2  update_stats per batch of 64 clips of 157 classes, 30 clips per video.  A: the host TestMeter(multi_label=True) fed
     with device predictions (one .cpu() and the Python loop per clip).  B: DeviceTestMeter(multi_label=True).
  3  The BCE loss at [8,157], forward and backward.  A: F.binary_cross_entropy_with_logits.  B: ops.bce_with_logits.  With the
     number of kernel launches of one forward + backward of each, from torch.profiler.
  4  The counting kernel alone (device time from the profiler's kernel records) at both sizes, the comparisons it makes --
     N per positive row of a wave that has a positive, counted on the host from the labels -- and the share of the
     integer issue rate that is: per comparison the loop issues about 5 VALU instructions (compare, two conditional adds,
     the label mask, its share of the LDS reads), 256 CUs x 4 SIMDs x 32 lanes per clock at the 2.4 GHz maximum clock.

No figure is gated: the tool reports what it finds."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def wall(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3                              # ms per call


def alternate(say, what, a, b, rounds, reps):
    for _ in range(2):
        a(), b()
    ta, tb = [], []
    for r in range(rounds):
        ta.append(wall(a, reps))
        tb.append(wall(b, reps))
        say("    round %d   A %9.4f ms   B %9.4f ms" % (r, ta[-1], tb[-1]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say("  %s: A median %.4f ms (min %.4f max %.4f), B median %.4f ms (min %.4f max %.4f), A / B = %.2f" % (
        what, ma, min(ta), max(ta), mb, min(tb), max(tb), ma / mb))
    return ma, mb


def tables(N, C, p, dev, seed):
    g = np.random.RandomState(seed)
    s = g.rand(N, C).astype(np.float32)
    y = (g.rand(N, C) < p).astype(np.float32)
    return torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)


def host_map(host_ap):
    def run(s, y):
        s, y = s.cpu().numpy(), y.cpu().numpy()
        keep = ~np.all(y == 0, axis=0)
        return float(np.mean(host_ap(y[:, keep], s[:, keep])))
    return run


def kernel_time(fn, kernel, iters=10):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    d = [getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in prof.events() if kernel in e.name]
    return (statistics.median(d) if d else float("nan")), len(d)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memcpy" not in e.name
             and "Memset" not in e.name]
    return len(names), sorted(set(n[:60] for n in names))


def comparisons(y):
    """What ap_count_kernel compares: N per row of every wave (64 consecutive rows of a class) that holds a positive."""
    N, C = y.shape
    pad = np.zeros((-(-N // 64) * 64, C), dtype=bool)
    pad[:N] = y == 1
    waves = pad.reshape(-1, 64, C).any(axis=1)
    return int(waves.sum()) * 64 * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilabel_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multilabel_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from focus_amd import ops
    from focus_amd.slowfast.utils import meters
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        from sklearn.metrics import average_precision_score
        host_ap = lambda y, s: average_precision_score(y, s, average=None)
        say("multilabel_bench on %s; host arm: scikit-learn average_precision_score" % torch.cuda.get_device_name(0))
    except ImportError:
        host_ap = lambda y, s: meters._average_precision_columns(s, y)
        say("multilabel_bench on %s; host arm: the numpy restatement of scikit-learn (scikit-learn is absent)" %
            torch.cuda.get_device_name(0))

    say("1  get_map of a device table: A = .cpu().numpy() + host average precision, B = focus_average_precision + one copy")
    run_a = host_map(host_ap)
    sizes = (("Charades test 1863 x 157, 4 % positives", 1863, 157, 0.04, 10), ("tool table 100000 x 7, 30 % positives", 100000, 7, 0.3, 2))
    kept = {}
    for what, N, C, p, reps in sizes:
        s, y = tables(N, C, p, dev, N)
        a, b = run_a(s, y), float(meters.get_map(s, y))
        say("  %s: host %.17g device %.17g difference %.3g" % (what, a, b, abs(a - b)))
        alternate(say, what, lambda: run_a(s, y), lambda: meters.get_map(s, y), args.rounds, reps)
        kept[what] = (s, y)

    say("2  update_stats per batch of 64 clips x 157 classes, 30 clips per video, 'max': A = host TestMeter, B = DeviceTestMeter")
    NV, NC, C = 1863, 30, 157
    g = torch.Generator().manual_seed(0)
    preds = torch.rand(64, C, generator=g).to(dev)
    ids = torch.arange(64) * 7 % (NV * NC)
    vlab = (torch.rand(NV, C, generator=g) < 0.04).float()
    labels = vlab[ids // NC]
    host = meters.TestMeter(NV, NC, C, 1, multi_label=True, ensemble_method="max")
    devm = meters.DeviceTestMeter(NV, NC, C, 1, dev, ensemble_method="max", multi_label=True)
    alternate(say, "update_stats", lambda: host.update_stats(preds, labels, ids), lambda: devm.update_stats(preds, labels, ids),
              args.rounds, 20)

    say("3  BCE with logits at [8,157], forward + backward: A = F.binary_cross_entropy_with_logits, B = ops.bce_with_logits")
    x = torch.randn(8, C, generator=g).to(dev).requires_grad_(True)
    t = (torch.rand(8, C, generator=g) < 0.04).float().to(dev)

    def step(fn):
        x.grad = None
        fn(x, t).backward()
    fa = lambda: step(lambda a, b: torch.nn.functional.binary_cross_entropy_with_logits(a, b))
    fb = lambda: step(lambda a, b: ops.bce_with_logits(a, b, "mean"))
    alternate(say, "BCE fwd + bwd", fa, fb, args.rounds, 200)
    for name, fn in (("A", fa), ("B", fb)):
        n, names = launches(fn)
        say("    %s: %d kernel launches per forward + backward: %s" % (name, n, "; ".join(names)))

    say("4  ap_count_kernel alone")
    for what, (s, y) in kept.items():
        us, n = kernel_time(lambda: ops.average_precision(s, y), "ap_count_kernel")
        cmp_ = comparisons(y.cpu().numpy())
        rate = cmp_ / (us * 1e-6) if us == us else float("nan")
        peak = 256 * 4 * 32 * 2.4e9 / 5
        say("  %s: median %.1f us over %d launches; %.3g comparisons, %.3g per second = %.0f %% of the integer issue rate at 5 "
            "instructions per comparison (%.3g / s)" % (what, us, n, cmp_, rate, 100 * rate / peak, peak))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
