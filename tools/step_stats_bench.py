"""Per-step statistics of the training loop: what the parent offers (the host NaN check, metrics.topk_errors and one
.item() per logged number, every step) against meters.StepStats (one kernel launch per step, one read every 10 steps).

    python tools/step_stats_bench.py [--rounds 4] [--steps 50] [--out profiles/step_stats_bench.txt]

Setup: the ORViT-MF 16x224 model of bench.py:make_cfg, batch 8, train.synthetic_batch resident in HBM, train.train_iter with
the fused optimizer.  One model and one optimizer serve both sides (the sides differ only in what they do with the
predictions).

  A  check_nan=True + metrics.topk_errors(preds, labels, (1, 5)) + .item() of top-1, top-5 and the loss, per step
  B  stats=StepStats, stats.read() every 10 steps

Both are warmed up, then rounds alternate A, B, A, B...; a round is `--steps` steps inside a wall clock that ends in a device
synchronise.  Every round is printed.  Gate: B's median step time is at most A's median plus A's own max - min.

A second, ungated pair does the same for the EPIC-Kitchens heads (97 verbs, 300 nouns) with mixup: A collapses the dense
labels (train.mixup_collapse inside train_iter) and reads verb / noun / action top-1 / top-5 and the loss through .item();
B hands the dense labels to the kernel.  Then the two kernels alone (the host's pace by HIP events, and the kernels' own device time from the profiler's kernel
records), and the count of device-to-host copies and scalar reads in a torch.profiler run of 10 steps of each side, B
without a read."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def setup(ek, dev):
    import bench
    from focus_amd import train
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    cfg = bench.make_cfg(1, 8)
    if ek:
        cfg.merge_from_list(["TRAIN.DATASET", "epickitchens", "MODEL.LOSS_FUNC", "soft_cross_entropy", "MIXUP.ENABLE", True])
    torch.manual_seed(0)
    np.random.seed(0)
    model = build_model(cfg, gpu_id=dev.index)
    model.train()
    opt = construct_optimizer(model, cfg)
    loss_fun = get_loss_func(cfg)(reduction="mean")
    inputs, labels, meta = train.synthetic_batch(cfg, 8, dev, seed=0)
    return dict(cfg=cfg, model=model, opt=opt, loss_fun=loss_fun, inputs=inputs, labels=labels, meta=meta,
                mixup=train.build_mixup(cfg), ek=ek)


def steps_a(s, n):
    """The parent's loop body; returns the last step's numbers."""
    from focus_amd import train
    from focus_amd.slowfast.utils import metrics
    out = None
    for _ in range(n):
        preds, labels, loss = train.train_iter(s["model"], s["opt"], s["loss_fun"], list(s["inputs"]), s["labels"], s["meta"],
                                               s["cfg"], mixup_fn=s["mixup"], check_nan=True)
        if s["ek"]:
            v = metrics.topk_accuracies(preds["verb"], labels["verb"], (1, 5))
            nn = metrics.topk_accuracies(preds["noun"], labels["noun"], (1, 5))
            a = metrics.multitask_topk_accuracies((preds["verb"], preds["noun"]), (labels["verb"], labels["noun"]), (1, 5))
            out = [x.item() for x in v] + [x.item() for x in nn] + [x.item() for x in a] + [loss.item()]
        else:
            e = metrics.topk_errors(preds, labels, (1, 5))
            out = [e[0].item(), e[1].item(), loss.item()]
    return out


def steps_b(s, n, stats, every=10):
    from focus_amd import train
    out = None
    for i in range(n):
        train.train_iter(s["model"], s["opt"], s["loss_fun"], list(s["inputs"]), s["labels"], s["meta"], s["cfg"],
                         mixup_fn=s["mixup"], stats=stats)
        if (i + 1) % every == 0:
            out = stats.read()
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pair(s, rounds, steps, say, multitask):
    from focus_amd.slowfast.utils import meters
    stats = meters.StepStats(s["inputs"][0].device, multitask=multitask)
    steps_a(s, 5)
    steps_b(s, 10, stats)
    ta, tb = [], []
    for r in range(rounds):
        ta.append(wall(lambda: steps_a(s, steps)) / steps * 1e3)
        tb.append(wall(lambda: steps_b(s, steps, stats)) / steps * 1e3)
        say("    round %d: A %.3f ms/step   B %.3f ms/step" % (r, ta[-1], tb[-1]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say("    A median %.3f ms/step (min %.3f, max %.3f)   B median %.3f ms/step (min %.3f, max %.3f)   B - A = %+.3f ms" % (
        ma, min(ta), max(ta), mb, min(tb), max(tb), mb - ma))
    return ta, tb


def d2h_count(s, multitask):
    """Device-to-host copies and scalar reads in 10 B steps without a read, and in 10 A steps, by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    from focus_amd.slowfast.utils import meters
    stats = meters.StepStats(s["inputs"][0].device, multitask=multitask)
    names = ("aten::item", "aten::_local_scalar_dense")
    out = []
    for fn in (lambda: steps_b(s, 10, stats, every=1000), lambda: steps_a(s, 10)):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = prof.events()
        # the runtime's name for a blocking device-to-host copy differs between builds: count every spelling, and keep the
        # names of all copy events so that the output shows what was matched against
        low = [e.name.lower() for e in ev]
        copies = sum(1 for n in low if ("memcpy" in n or "copy" in n) and ("dtoh" in n or "devicetohost" in n or "d2h" in n))
        seen = sorted({e.name for e in ev if "memcpy" in e.name.lower()})
        out.append((copies, sum(1 for e in ev if e.name == names[0]), sum(1 for e in ev if e.name == names[1]), seen))
    stats.read()
    return out


def report_d2h(counts, say):
    for what, (c, i, d, seen) in zip(("10 steps of B without a read:", "10 steps of A:               "), counts):
        say("    %s %d device-to-host copies, %d aten::item, %d aten::_local_scalar_dense; copy events seen: %s" % (
            what, c, i, d, ", ".join(seen) or "none"))


def kernel_times(dev, say):
    from focus_amd import ops

    def timed(fn, kernel, iters=50):
        """(host-paced time per call from HIP events, the kernel's own device time from the profiler's kernel records), us."""
        from torch.profiler import ProfilerActivity, profile
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        d = [getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in prof.events() if kernel in e.name]
        return a.elapsed_time(b) / iters * 1e3, (statistics.median(d) if d else float("nan")), len(d)

    fmt = "%.1f us per call when issued back to back (the host's pace); kernel alone: median %.1f us over %d launches"
    acc_i = torch.zeros(ops.STATS_INTS, dtype=torch.int64, device=dev)
    acc_f = torch.zeros(ops.STATS_FLOATS, dtype=torch.float64, device=dev)
    g = torch.Generator().manual_seed(0)
    loss = torch.zeros((), device=dev)
    x = torch.randn(8, 174, generator=g).to(dev).to(torch.bfloat16)
    l = torch.randint(0, 174, (8,), generator=g).to(dev)
    say("    focus_topk_stats  B=8 V=174 bf16, int labels:          " + fmt %
        timed(lambda: ops.topk_stats(acc_i, acc_f, x, l, (1, 5), [loss]), "topk_stats_kernel"))
    v, n = torch.randn(8, 97, generator=g).to(dev).to(torch.bfloat16), torch.randn(8, 300, generator=g).to(dev).to(torch.bfloat16)
    dv, dn = torch.rand(8, 97, generator=g).to(dev), torch.rand(8, 300, generator=g).to(dev)
    say("    focus_topk_stats  B=8 V=(97,300) bf16, dense labels:   " + fmt %
        timed(lambda: ops.topk_stats(acc_i, acc_f, (v, n), (dv, dn), (1, 5), [loss, loss, loss]), "topk_stats_kernel"))
    NV, NC, C = 1000, 30, 174
    table = torch.zeros(NV, C, device=dev)
    tl, cc = torch.zeros(NV, dtype=torch.int64, device=dev), torch.zeros(NV, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    p = torch.rand(64, C, generator=g).to(dev)
    ids, lab = torch.arange(64, device=dev), torch.ones(64, dtype=torch.int64, device=dev)
    say("    focus_view_accumulate  n=64 C=174 fp32, 30 clips/video: " + fmt %
        timed(lambda: ops.view_accumulate(p, ids, lab, NC, table, tl, cc, flag), "view_accumulate_kernel"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_stats_bench: needs the MI355X (timings from a CPU say nothing about it)")
    if args.rounds < 4 or args.steps < 50:
        raise SystemExit("step_stats_bench: at least 4 rounds of at least 50 steps")
    dev = torch.device("cuda:0")
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("ORViT-MF 16x224, batch 8, bf16 storage, fused optimizer; %d rounds x %d steps per side, alternated, wall clock" % (
        args.rounds, args.steps))
    say("1. Ssv2 head (174 classes): A = check_nan + topk_errors + 3 x .item() per step; B = StepStats, read every 10 steps")
    s = setup(False, dev)
    ta, tb = pair(s, args.rounds, args.steps, say, False)
    ma, mb = statistics.median(ta), statistics.median(tb)
    ok = mb <= ma + (max(ta) - min(ta))
    say("    gate: B median %.3f <= A median %.3f + A spread %.3f: %s" % (mb, ma, max(ta) - min(ta), "PASS" if ok else "FAIL"))
    report_d2h(d2h_count(s, False), say)
    del s
    torch.cuda.empty_cache()
    say("2. EPIC-Kitchens heads (97 + 300) with mixup, not gated: A = check_nan + mixup_collapse + 7 x .item() per step; B = StepStats")
    s = setup(True, dev)
    pair(s, args.rounds, args.steps, say, True)
    report_d2h(d2h_count(s, True), say)
    del s
    torch.cuda.empty_cache()
    say("3. the kernels alone")
    kernel_times(dev, say)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
