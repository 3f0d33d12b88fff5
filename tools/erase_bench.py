"""Random erasing on the device: datasets.device_sampling.erase_clips (one launch of csrc/random_erase.hip) against the
reference's own expressions, at the batch of the shipped ORViT configs.

    python tools/erase_bench.py [--rounds 12] [--iters 10] [--out FILE]

Workload: a [8,3,16,224,224] batch in fp32 and in bf16, AUG.RE_PROB 1 (every clip erased), RE_MODE pixel, RE_COUNT 1.  Every
arm plans with the reference's draws from the same random.seed, so all arms erase the same rectangles:
  erase_clips   the planning of 8 clips on the host, one H2D copy of the table, the seed draw, one launch;
  ATen on GPU   the reference's expressions on the same device tensor: per clip and frame the slice assignment of
                torch.empty((C, h, w), device="cuda").normal_()  (random_erasing.py:18-31, :145-155);
  host path     what the reference does with a device batch today: D2H, its RandomErasing on the CPU tensor, H2D.
Whole calls, timed with the host clock around `iters` calls that end in a device synchronise (so host-bound calls show as
such), after a warm-up, the arms alternating round by round; median, min and max over the rounds.  Then the kernel alone
(table and seed already on the device), timed with device events, in mode pixel and in mode const (the same stores without
the draws): its time and the bytes it writes per second against the HBM peak (8 TB/s; about 6.3 TB/s achievable)."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.config.defaults import get_cfg  # noqa: E402
from focus_amd.slowfast.datasets import device_sampling as ds  # noqa: E402
from focus_amd.slowfast.datasets.random_erasing import RandomErasing  # noqa: E402

SHAPE = (8, 3, 16, 224, 224)
HBM_PEAK = 8.0e12


def make_cfg(mixed):
    cfg = get_cfg()
    cfg.merge_from_list(["AUG.ENABLE", True, "AUG.RE_PROB", 1.0, "AUG.RE_MODE", "pixel", "AUG.RE_COUNT", 1,
                         "MODEL.MODEL_NAME", "Motionformer", "TRAIN.MIXED_PRECISION", mixed])
    return cfg


def transform():
    return RandomErasing(1.0, mode="pixel", max_count=1, num_splits=1, device="cpu")


def plans():
    return [transform().plan(SHAPE[2], SHAPE[3], SHAPE[4]) for _ in range(SHAPE[0])]


def aten_on_gpu(x):
    for b, items in enumerate(plans()):
        for it in items:
            for t in range(it["t0"], it["t1"]):
                x[b, :, t, it["top"]:it["top"] + it["h"], it["left"]:it["left"] + it["w"]] = torch.empty(
                    (SHAPE[1], it["h"], it["w"]), dtype=x.dtype, device=x.device).normal_()
    return x


def host_path(x):
    h = x.cpu()
    for b in range(h.shape[0]):
        transform()(h[b].permute(1, 0, 2, 3))                             # ssv2.py:444-446
    return h.to(x.device)


def wall(fn, x, iters, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        random.seed(seed + i)
        fn(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6                        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("erase_bench: needs the MI355X (timings from a CPU say nothing about it)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("batch %s, RE_PROB 1, pixel, RE_COUNT 1; %d rounds x %d calls (host path: %d), alternated" % (
        list(SHAPE), args.rounds, args.iters, max(1, args.iters // 5)))
    for mixed, dname in ((False, "fp32"), (True, "bf16")):
        cfg = make_cfg(mixed)
        dtype = torch.bfloat16 if mixed else torch.float32
        x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(1)).to(dtype).cuda()
        arms = (("erase_clips", lambda t: ds.erase_clips(cfg, t), args.iters), ("ATen on GPU", aten_on_gpu, args.iters),
                ("host path", host_path, max(1, args.iters // 5)))
        for _name, fn, n in arms:                                          # warm-up of every arm
            wall(fn, x, min(n, 3), 0)
        times = {name: [] for name, _f, _n in arms}
        for r in range(args.rounds):
            for name, fn, n in arms:
                times[name].append(wall(fn, x, n, 1000 * r))
        say("%s, whole calls:" % dname)
        for name, _f, _n in arms:
            t = times[name]
            say("  %-12s median %9.1f us   min %9.1f   max %9.1f" % (name, statistics.median(t), min(t), max(t)))
        for name in ("ATen on GPU", "host path"):
            ratio = [a / b for a, b in zip(times[name], times["erase_clips"])]
            say("  %s / erase_clips per round: median %.1fx, min %.1fx, max %.1fx" % (
                name, statistics.median(ratio), min(ratio), max(ratio)))

        # the kernel alone: one table for the whole measurement
        random.seed(0)
        items = [dict(it, clip=b) for b, its in enumerate(plans()) for it in its]
        rec, most = ops.erase_table(items, SHAPE[0], SHAPE[2], SHAPE[3], SHAPE[4])
        table = torch.from_numpy(rec).cuda()
        seed = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
        plane = SHAPE[3] * SHAPE[4]
        written = sum(SHAPE[1] * (it["t1"] - it["t0"]) * it["h"] * it["w"] for it in items) * x.element_size()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def kernel(mode):
            _lib.check(_lib.lib().focus_random_erase(
                ctypes.c_void_p(x.data_ptr()), _lib.BF16 if mixed else _lib.F32, SHAPE[0], SHAPE[2], SHAPE[1], SHAPE[3], SHAPE[4],
                SHAPE[1] * SHAPE[2] * plane, SHAPE[2] * plane, plane, ctypes.c_void_p(table.data_ptr()), rec.shape[0], most,
                ops.ERASE_MODES.index(mode), ctypes.c_void_p(seed.data_ptr()), stream), "random_erase")
        say("  kernel alone (50 back-to-back launches per round, device events), writing %.2f MB in %d rectangles:" % (
            written / 1e6, len(items)))
        for mode in ("pixel", "const"):                                     # const: the store path without the draws
            for _ in range(20):
                kernel(mode)
            tk = []
            for _ in range(args.rounds):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(50):
                    kernel(mode)
                e.record()
                e.synchronize()
                tk.append(s.elapsed_time(e) / 50 * 1e3)
            med = statistics.median(tk)
            say("    %-5s median %5.1f us   min %5.1f   max %5.1f   %.2f TB/s, %.0f%% of the %.0f TB/s HBM peak" % (
                mode, med, min(tk), max(tk), written / med / 1e6, 100.0 * written / (med * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
