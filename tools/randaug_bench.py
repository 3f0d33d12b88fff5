"""Device RandAugment: datasets/device_sampling.augment_clips (host planner + ops.randaug_apply -> csrc/randaug.hip) at the batch
of the shipped ORViT configs, and for context the host time of the same plans through PIL.

    python tools/randaug_bench.py [--rounds 7] [--iters 10] [--out FILE]

Workload: 8 clips of 16 x 240 x 427 uint8 frames under AUG.AA_TYPE rand-m7-n4-mstd0.5-inc1, DIFFERENT_AUG_PER_FRAME,
INTERPOLATION bicubic: 128 frames, four layers, a fresh draw per frame.  Every call is re-seeded, so all calls run the same
plans.  Three things are timed, alternating round by round, and the spread over the rounds is printed beside the medians:
  augment_clips    the whole call: the host draws and box moves of 128 plans, the table copy, the launches, to a device
                   synchronise (host clock);
  randaug_apply    the same plans prebuilt: the H2D table copy and the launches only (device events);
  layers           each layer's launches alone through the C ABI on a table already on the device (device events over
                   --iters calls, the workspace zeroed before each as randaug_apply zeroes it once): kernel time plus
                   launch gaps, the figure the bytes/s of the kernels are taken over;
  PIL              the same plans on the host through PIL, one thread, frames converted from and to numpy as a loader worker
                   would (host clock); only when PIL imports.
The device result is compared with PIL's byte for byte first.  Bytes are the algorithm's: per layer one read and one write of
every frame, plus one more read of the frames whose op needs the histogram or the mean; over the event time of a
layer's launches.  The 94 MB of clips (input, output, scratch) fit the 256 MiB Infinity Cache, so the rates are not HBM rates."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.config.defaults import get_cfg  # noqa: E402
from focus_amd.slowfast.datasets import device_sampling, transform  # noqa: E402
from focus_amd.slowfast.datasets import rand_augment as ra  # noqa: E402

B, T, H, W = 8, 16, 240, 427
POLICY = "rand-m7-n4-mstd0.5-inc1"
SEED = 20271
HBM_PEAK = 8.0e12                     # bytes/s, the MI355X's specified peak


def seed_all():
    random.seed(SEED)
    np.random.seed(SEED)


def make_cfg():
    cfg = get_cfg()
    cfg.merge_from_list(["AUG.ENABLE", "True", "AUG.AA_TYPE", POLICY, "AUG.DIFFERENT_AUG_PER_FRAME", "True",
                         "AUG.INTERPOLATION", "bicubic"])
    return cfg


def make_clips():
    rng = np.random.RandomState(3)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255) // (W - 1), (y * 255) // (H - 1), ((x + y) * 255) // (H + W - 2)], -1)
    return [np.clip(base[None] * 0.7 + rng.randint(0, 70, (T, H, W, 3)) + 5 * b, 0, 255).astype(np.uint8) for b in range(B)]


def build_plans():
    seed_all()
    return [[transform.create_random_augment((H, W), POLICY, "bicubic").plan((W, H))[0] for _ in range(T)] for _ in range(B)]


def pil_apply(img, rec):
    from PIL import Image, ImageEnhance, ImageOps
    if rec is None:
        return img
    op, f, i = rec["op"], rec["farg"], rec["iarg"]
    if op in ra.AFFINE_OPS:
        if rec["coef"] is None:
            return img.copy()
        return img.transform(img.size, Image.AFFINE, rec["coef"], resample=rec["resample"][0], fillcolor=rec["fill"])
    if op == ra.OP_AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if op == ra.OP_EQUALIZE:
        return ImageOps.equalize(img)
    if op == ra.OP_INVERT:
        return ImageOps.invert(img)
    if op == ra.OP_POSTERIZE:
        return img if i >= 8 else ImageOps.posterize(img, i)
    if op == ra.OP_SOLARIZE:
        return ImageOps.solarize(img, i)
    if op == ra.OP_SOLARIZE_ADD:
        return img.point([min(255, v + i) if v < 128 else v for v in range(256)] * 3)
    enh = {ra.OP_BRIGHTNESS: ImageEnhance.Brightness, ra.OP_COLOR: ImageEnhance.Color, ra.OP_CONTRAST: ImageEnhance.Contrast,
           ra.OP_SHARPNESS: ImageEnhance.Sharpness}[op]
    return enh(img).enhance(f)


def pil_batch(clips, plans):
    from PIL import Image
    out = []
    for clip, pl in zip(clips, plans):
        frames = []
        for t in range(T):
            img = Image.fromarray(clip[t])
            for rec in pl[t]:
                img = pil_apply(img, rec)
            frames.append(np.asarray(img))
        out.append(np.stack(frames))
    return out


def layer_times(dev, plans, args, say):
    """Each layer's stats + apply launches alone, on a device table, against the bytes the layer moves."""
    t = ops.randaug_table(dev, plans)
    rec, L = t["rec"], _lib.lib()
    n, size = rec.shape[1], rec.dtype.itemsize
    ws_bytes = int(L.focus_randaug_workspace_bytes(t["n_stats"]))
    ws = torch.zeros(max(ws_bytes // 4, 2), dtype=torch.int32, device="cuda")
    items = torch.from_numpy(rec.reshape(-1).view(np.uint8)).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(l):
        ws.zero_()
        _lib.check(L.focus_randaug_layer(ctypes.c_void_p(items.data_ptr() + l * n * size), n, t["max_h"], t["max_w"],
                                         int(t["need_stats"][l]), ctypes.c_void_p(ws.data_ptr()), ws_bytes, stream), "randaug_layer")

    for l in range(rec.shape[0]):
        for _ in range(3):
            launch(l)
        times = []
        for _ in range(args.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                launch(l)
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e) / args.iters * 1e3)
        ops_l = rec[l]["op"]
        n_st = int(np.isin(ops_l, ops.RANDAUG_STAT_OPS).sum())
        nbytes = int((2 * n + n_st) * H * W * 3)
        med = statistics.median(times)
        say("    layer %d (%3d copies, %3d table, %3d blend, %3d affine; %s)  median %7.1f us  min %7.1f  max %7.1f   %.2f TB/s of"
            " %.1f MB = %.0f %% of the %.1f TB/s HBM peak" % (
                l, int((ops_l == 0).sum()), int(((ops_l >= 1) & (ops_l <= 7)).sum()), int(((ops_l >= 8) & (ops_l <= 10)).sum()),
                int((ops_l >= 11).sum()), "stats + apply" if t["need_stats"][l] else "apply only", med, min(times), max(times),
                nbytes / med / 1e6, nbytes / 1e6, 100 * nbytes / (med * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench: needs the MI355X (timings from a CPU say nothing about it)")
    try:
        import PIL
        have_pil = PIL.__version__
    except ImportError:
        have_pil = None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg, host = make_cfg(), make_clips()
    dev = [torch.from_numpy(c).cuda() for c in host]
    plans = build_plans()
    recs = [r for pl in plans for fr in pl for r in fr]
    n_open = sum(r is not None for r in recs)
    n_stats = sum(r is not None and r["op"] in ops.RANDAUG_STAT_OPS for r in recs)
    n_affine = sum(r is not None and r["op"] in ops.RANDAUG_AFFINE_OPS and r["coef"] is not None for r in recs)
    frame_bytes = H * W * 3
    moved = (2 * len(recs) + n_stats) * frame_bytes
    say("device: %s" % torch.cuda.get_device_name(0))
    say("batch %d x %d x %dx%d uint8, policy %s, per-frame draws, bicubic; %d rounds x %d calls, alternated" % (
        B, T, H, W, POLICY, args.rounds, args.iters))
    say("plans: %d frame-layers, %d with an open gate (%d affine, %d needing the stats launch); %.1f MB moved per call" % (
        len(recs), n_open, n_affine, n_stats, moved / 1e6))

    def whole():
        seed_all()
        out = device_sampling.augment_clips(cfg, dev, None)[0]
        torch.cuda.synchronize()
        return out

    def apply_only():
        return ops.randaug_apply(dev, plans)

    got = whole()
    same_plans = all(torch.equal(a, b) for a, b in zip(got, apply_only()))
    say("augment_clips from the seed == randaug_apply on the prebuilt plans: %s" % same_plans)
    if have_pil:
        want = pil_batch(host, plans)
        diff = sum(int((g.cpu().numpy() != w).any(-1).sum()) for g, w in zip(got, want))
        say("device output vs PIL %s on the same plans: %d of %d pixels differ" % (have_pil, diff, B * T * H * W))
    for _ in range(3):
        whole()
        apply_only()
    torch.cuda.synchronize()
    t_whole, t_apply, t_pil = [], [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            whole()
        t_whole.append((time.perf_counter() - t0) / args.iters * 1e6)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            apply_only()
        e.record()
        e.synchronize()
        t_apply.append(s.elapsed_time(e) / args.iters * 1e3)
        if have_pil:
            t0 = time.perf_counter()
            pil_batch(host, plans)
            t_pil.append((time.perf_counter() - t0) * 1e6)
    fmt = "  %-34s median %10.1f us   min %10.1f   max %10.1f"
    say(fmt % ("augment_clips (whole call, host clock)", statistics.median(t_whole), min(t_whole), max(t_whole)))
    say(fmt % ("randaug_apply (prebuilt plans, events)", statistics.median(t_apply), min(t_apply), max(t_apply)))
    layer_times(dev, plans, args, say)
    if have_pil:
        say(fmt % ("PIL on the host, one thread", statistics.median(t_pil), min(t_pil), max(t_pil)))
        ratio = [p / w for p, w in zip(t_pil, t_whole)]
        say("  PIL / augment_clips per round: median %.1fx, min %.1fx, max %.1fx (PIL alone; the reference's loader also"
            " copies the clip to the device afterwards)" % (statistics.median(ratio), min(ratio), max(ratio)))
    else:
        say("  PIL does not import here: host side not measured")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
